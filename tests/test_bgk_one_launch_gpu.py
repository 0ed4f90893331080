"""The one-launch BGK scan (bgk_predict_fuse_t1, la3dm_amd/csrc/bgk_scan1_kernels.h; option "bgk_one_launch" 1, the default) against
the two launches it replaces (bgk_prepare + bgk_predict_fuse_t<.., false>; "bgk_one_launch" 0) in the same build, through the C ABI
(la3dm_bgk_scan_host) on the same packed scans.  Both kernels add the same fp32 terms in the same order into the same double
accumulators — the scaled coordinates are the same correctly rounded quotients, the neighbour descriptor holds the same thirteen
words — so alpha, beta and state have to be EQUAL BIT FOR BIT, not merely close.

The one-launch path is taken for full-block table scans at block_depth 3 only; which path a call took is read from the
counters it returns (scratch_bytes: 0 for the one launch, 16 bytes per training point for the prescale pass)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAYS = 3000   # smallest round count whose packed scan has test blocks in every class of M below (checked on the CPU: prepare() needs no device)
ELL_ALL_ONES = 0.24999998509883881   # fp32 0x3E7FFFFF: significand all ones, so the context keeps inv_ell = 0 and div_by_ell divides


def _flat_counts(pk):
    """M of every test block: the points of its 7 neighbour models together."""
    cnt = np.diff(pk.train_off.astype(np.int64))
    return np.where(pk.nbr >= 0, cnt[np.maximum(pk.nbr, 0)], 0).sum(axis=1)


def _fresh(depth=3, rays=RAYS, earlier=0, **over):
    import la3dm_amd
    params = dict(la3dm_amd.BGK_YAML, block_depth=depth, **over)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    m = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(False)
    m.set_option("bgk_sum", 1)
    for s in range(earlier):
        assert m.prepare(xyz + np.float32(0.013 * (s + 1)), origin, 0.1, 0.5, -1.0)
        m.scan_host(m.packed())
        m.commit()
    assert m.prepare(xyz, origin, 0.1, 0.5, -1.0)
    pk = m.packed()
    assert pk.flags & 2          # LA3DM_SCAN_LABELS_01 from the front end
    return m, pk


@pytest.fixture(scope="module")
def scan(built):
    """a fresh depth-3 map's first scan, packed; the tests restore whatever they change in it"""
    m, pk = _fresh()
    assert pk.flags & 4 and int(pk.n_leaf) == int(pk.n_test_blk) * 64     # every block full
    return m, pk, pk.alpha.copy(), pk.beta.copy(), pk.nbr.copy()


def _run(m, pk, a0, b0, flags, one, scans=1):
    """the scan `scans` times in a row from (a0, b0); returns the outputs after every scan and whether the one launch ran"""
    m.set_option("bgk_one_launch", one)
    assert m.get_option("bgk_one_launch") == one
    pk.alpha[:], pk.beta[:], pk.c.flags = a0, b0, flags
    out, took = [], []
    for _ in range(scans):
        pk.state[:] = 0x55    # (neither a state nor 0: a leaf that a kernel leaves untouched shows)
        cnt = m.scan_host(pk)
        took.append(int(cnt.scratch_bytes) == 0)
        out.append((pk.alpha.copy(), pk.beta.copy(), pk.state.copy()))
    assert len(set(took)) == 1
    return out, took[0]


def _assert_same_bits(ref, new):
    assert len(ref) == len(new)
    for r, n in zip(ref, new):
        for name, x, y in zip(("alpha", "beta", "state"), r, n):
            differ = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.dtype == np.uint8 else int((x.view(np.uint32) != y.view(np.uint32)).sum())
            print(f"{name}: {differ} of {x.size} differ")
            assert differ == 0, name


def _both(m, pk, a0, b0, flags, scans=1, expect_one=True):
    ref, took0 = _run(m, pk, a0, b0, flags, 0, scans)
    new, took1 = _run(m, pk, a0, b0, flags, 1, scans)
    m.set_option("bgk_one_launch", 1)
    pk.alpha[:], pk.beta[:], pk.c.flags = a0, b0, flags
    assert not took0 and took1 == expect_one
    _assert_same_bits(ref, new)
    return new


def _doctor(pk, M):
    """rewrites rows of pk.nbr in place; returns the rows it emptied"""
    n = pk.nbr.shape[0]
    have_self = np.flatnonzero((pk.nbr[:, 0] >= 0) & ((pk.nbr[:, 1:] >= 0).sum(axis=1) >= 2))
    assert have_self.size >= 64
    heavy = have_self[np.argsort(-M[have_self], kind="stable")]     # the busiest first: rows whose change moves many sums
    empty = np.concatenate([heavy[0:48:3], [n - 1]])                 # all -1: M = 0 (the LAST row of the array among them)
    assert pk.nbr[0, 0] >= 0 and (pk.nbr[0, 1:] >= 0).any()
    only_self = np.concatenate([heavy[1:48:3], [0]])                 # the self entry only (the FIRST row of the array among them)
    no_self = heavy[2:48:3]
    pk.nbr[empty] = -1
    pk.nbr[only_self, 1:] = -1
    pk.nbr[no_self, 0] = -1
    # a -1 in the middle of a row whose entries on both sides stay
    mid = [r for r in heavy[48:] if r != 0 and pk.nbr[r, 2] >= 0 and pk.nbr[r, 3] >= 0 and pk.nbr[r, 4] >= 0]
    assert mid
    pk.nbr[mid[0], 3] = -1
    return empty


def test_scan_covers_every_chunk_count(scan):
    """M = the points of a test block's 7 neighbours: one chunk, two, three (the first that re-forms the offsets), more"""
    m, pk, a0, b0, nbr0 = scan
    M = _flat_counts(pk)
    for lo, hi in ((1, 63), (65, 128), (129, 192), (193, 1 << 30)):
        assert ((M >= lo) & (M <= hi)).any(), (lo, hi)


def test_plain_scan(scan):
    m, pk, a0, b0, nbr0 = scan
    new = _both(m, pk, a0, b0, pk.flags)
    assert (new[0][0] != a0).any()


def test_doctored_neighbour_rows(scan):
    """rows without any neighbour (M = 0), with the self entry only, without the self entry, with a hole in the middle; the first
    and the last row of the array among them"""
    m, pk, a0, b0, nbr0 = scan
    try:
        empty = _doctor(pk, _flat_counts(pk))
        M = _flat_counts(pk)
        assert (M[empty] == 0).all() and M[-1] == 0 and (pk.nbr[0] != nbr0[0]).any() and (pk.nbr[-1] != nbr0[-1]).any()
        new = _both(m, pk, a0, b0, pk.flags)
        assert (new[0][0] != a0).any()
        st = new[0][2].reshape(-1, 64)
        assert (st[empty] == 0).all()           # gated scan: a block nothing reaches is left alone, state 0
    finally:
        pk.nbr[:] = nbr0


def test_ungated_update(scan):
    """flags | 1 (insert_training_data): update() runs for every leaf, the leaves of M = 0 blocks included"""
    m, pk, a0, b0, nbr0 = scan
    flags = pk.flags
    try:
        empty = _doctor(pk, _flat_counts(pk))
        new = _both(m, pk, a0, b0, flags | 1)
        st = new[0][2].reshape(-1, 64)
        assert (st[empty] & 0x80).all()         # classified although nothing reached them
        assert (st & 0x80).all()
    finally:
        pk.nbr[:] = nbr0
        pk.c.flags = flags


def test_reinsertion(scan):
    """three scans in a row, alpha and beta carried over"""
    m, pk, a0, b0, nbr0 = scan
    new = _both(m, pk, a0, b0, pk.flags, scans=3)
    assert (new[2][0] != new[0][0]).any()


def test_ieee_division(built):
    """an ell whose significand is all ones: la3dm_create keeps inv_ell = 0 and div_by_ell takes the IEEE division"""
    assert int(np.float32(ELL_ALL_ONES).view(np.uint32)) & 0x7FFFFF == 0x7FFFFF and float(np.float32(ELL_ALL_ONES)) == ELL_ALL_ONES
    m, pk = _fresh(ell=ELL_ALL_ONES)
    a0 = pk.alpha.copy()
    new = _both(m, pk, a0, pk.beta.copy(), pk.flags)
    assert (new[0][0] != a0).any()


def test_fallbacks_take_the_two_launches(scan):
    """without LA3DM_SCAN_FULL_BLOCKS, without LA3DM_SCAN_LABELS_01, at block_depth 4 and on a scan with pruned blocks the option
    changes nothing: the two launches run (the counters say so) and give the same bits"""
    m, pk, a0, b0, nbr0 = scan
    flags = pk.flags
    try:
        _both(m, pk, a0, b0, flags & ~4, expect_one=False)
        _both(m, pk, a0, b0, flags & ~2, expect_one=False)
    finally:
        pk.c.flags = flags
    m4, pk4 = _fresh(depth=4, rays=1500)
    assert pk4.flags & 4
    _both(m4, pk4, pk4.alpha.copy(), pk4.beta.copy(), pk4.flags, expect_one=False)
    m3, pk3 = _fresh(earlier=2)
    assert int(pk3.n_leaf) != int(pk3.n_test_blk) * 64      # pruned blocks
    new = _both(m3, pk3, pk3.alpha.copy(), pk3.beta.copy(), pk3.flags, expect_one=False)
    assert (new[0][2] != 0x55).all()
