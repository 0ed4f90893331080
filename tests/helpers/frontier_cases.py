"""The yardstick, the cases and the input conditions shared by tests/test_frontier_cpu.py and tests/test_frontier_gpu.py.

The yardstick never calls frontier or box: the classes come from `region_cases.yardstick` (a walk of the leaf list) over a
region one voxel larger on every side than the one queried, so the class of every neighbour is known; the score is the
sum of up to 26 shifted slices of that array and the list is np.flatnonzero.

Run as a program (`python frontier_cases.py <out.npz>`) it is the child process of the GPU test for the scan's ticket form:
two scans into a device-resident map, the recipe query, the answer saved for the parent."""
import os
import sys

import numpy as np

if __name__ == "__main__":                               # the child process: what conftest.py does for the tests
    ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers")]

import region_cases as R  # noqa: E402

CONNECTIVITIES = (6, 18, 26)
FREE_M, OCC_M, UNK_M, MISS_M = 1 << R.FREE, 1 << R.OCCUPIED, 1 << R.UNKNOWN, 1 << R.MISSING
# (open, unknown): the planner's pair; the roles swapped onto known classes; overlapping masks; nearly everything
MASK_PAIRS = ((FREE_M, UNK_M | MISS_M), (OCC_M, FREE_M), (FREE_M | UNK_M, UNK_M | MISS_M), (0xF, 0x1E))
SHAPES = ((1, 1, 1), (1, 1, 41), (33, 1, 1), (5, 64, 1), (3, 5, 7))
WORD_SHAPES = ((1, 1, 31), (1, 1, 32), (1, 1, 33), (1, 1, 63), (1, 1, 64), (1, 1, 65), (2, 2, 64))   # word / wave boundaries
LONG_SHAPES = ((1, 1, 3000), (3000, 2, 2))
SHAPE_OFFSET = (37, 41, 14)                              # in the thick of the recipe region (distance_cases' anchor)


def offsets(connectivity):
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(di, dj, dk) for di in (-1, 0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1)
            if 1 <= abs(di) + abs(dj) + abs(dk) <= reach]


def in_mask(cls, mask):
    return ((np.uint32(mask) >> cls.astype(np.uint32)) & 1).astype(bool)


def score_of(pcls, open_mask, unknown_mask, connectivity):
    """dense score of the interior of the padded class array pcls (nx + 2, ny + 2, nz + 2): shifted slices, summed"""
    nx, ny, nz = (s - 2 for s in pcls.shape)
    unk = in_mask(pcls, unknown_mask).astype(np.uint8)
    c = np.zeros((nx, ny, nz), np.uint8)
    for di, dj, dk in offsets(connectivity):
        c += unk[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz]
    return np.where(in_mask(pcls[1:-1, 1:-1, 1:-1], open_mask), c, np.uint8(0)).astype(np.uint8)


def answer_of(score, min_neighbours, cap=None):
    index = np.flatnonzero(score.reshape(-1) >= min_neighbours).astype(np.uint32)
    n = int(index.size)
    if cap is not None:
        index = index[:cap]
    return dict(n=n, index=index, nbrs=score.reshape(-1)[index].astype(np.uint8), score=score)


def yardstick(pcls, open_mask, unknown_mask, connectivity, min_neighbours, cap=None):
    return answer_of(score_of(pcls, open_mask, unknown_mask, connectivity), min_neighbours, cap)


def padded_case(m, lv, big_lo, dims):
    """a region of `dims` anchored one voxel inside the yardstick region of dims + 2 at big_lo: (lo to query, padded
    classes, the info the query must return)"""
    depth, res = int(m.get_block_depth()), np.float32(m.get_resolution())
    big = tuple(int(d) + 2 for d in dims)
    y = R.yardstick(m, lv, big_lo, big)
    lo = (y["origin"] + np.float32(1) * res).astype(np.float32)
    return lo, y["cls"], advanced_info(y, depth)


def sub_case(y, offset, dims, res):
    """the same from an existing yardstick y: the sub-box of `dims` at `offset` (>= 1 on every axis, so its halo is known)"""
    assert all(o >= 1 and o + d + 1 <= s for o, d, s in zip(offset, dims, y["cls"].shape)), (offset, dims)
    lo = (y["origin"] + np.array(offset, np.float32) * np.float32(res)).astype(np.float32)
    sl = tuple(slice(o - 1, o + d + 1) for o, d in zip(offset, dims))
    return lo, np.ascontiguousarray(y["cls"][sl])


def advanced_info(y, depth, by=(1, 1, 1)):
    """block key and cell of the yardstick's anchor advanced by `by` voxels, in integers"""
    lim = 1 << (depth - 1)
    b = [(int(y["block_key"]) >> s) & 0xFFFFF for s in (40, 20, 0)]
    g = [bk * lim + int(c) + int(a) for bk, c, a in zip(b, y["cell"], by)]
    return dict(block_key=((g[0] // lim) << 40) | ((g[1] // lim) << 20) | (g[2] // lim), cell=np.array([v % lim for v in g], np.int32))


def interior(y, res):
    """the recipe's interior box: dims (78, 78, 38) one voxel inside the 80 x 80 x 40 yardstick region"""
    dims = tuple(s - 2 for s in y["cls"].shape)
    return sub_case(y, (1, 1, 1), dims, res) + (dims,)


def assert_same(got, want, what, fields=("index", "nbrs", "score")):
    """exact: n by ==, the arrays by == with shape and dtype"""
    assert got["n"] == want["n"], (what, got["n"], want["n"])
    R.assert_same(got, want, [k for k in fields if k in want and k in got], what)


def input_conditions(pcls):
    """counted from the yardstick's classes of the padded interior box, never from the code under test"""
    s = {c: score_of(pcls, FREE_M, UNK_M | MISS_M, c) for c in CONNECTIVITIES}
    front6 = s[6] >= 1
    face = np.zeros(front6.shape, bool)
    for ax in range(3):
        for side in (0, -1):
            sl = [slice(None)] * 3
            sl[ax] = side
            face[tuple(sl)] = True
    return dict(front6=int(front6.sum()), front18=int((s[18] >= 1).sum()), front26=int((s[26] >= 1).sum()),
                score3=int((s[26] >= 3).sum()), distinct=int(np.unique(s[26][s[26] >= 1]).size),
                faces=int((front6 & face).sum()), swapped=int((score_of(pcls, OCC_M, FREE_M, 26) >= 1).sum()))


def assert_exercises_the_feature(cond):
    """at least half of what was counted on region_cases.fused_map(3) (8 592 / 12 118 / 13 304 frontier voxels at
    connectivity 6 / 18 / 26, 10 702 with score >= 3, 23 distinct scores, 158 on the faces of the box, 3 112 with open =
    OCCUPIED and unknown = FREE): the margin the region tests use between that map and the product's"""
    print(f"frontier input conditions: {cond}")
    assert cond["front6"] >= 4296 and cond["front18"] >= 6059 and cond["front26"] >= 6652, cond
    assert cond["score3"] >= 5351 and cond["distinct"] >= 12 and cond["faces"] >= 79 and cond["swapped"] >= 1556, cond


def long_line_lo(y, resolution, dims):
    """distance_cases.long_line_lo for the padded line: the anchor of the yardstick region of dims + 2"""
    import distance_cases as D
    return D.long_line_lo(y, resolution, tuple(d + 2 for d in dims))


if __name__ == "__main__":
    import la3dm_amd
    from conftest import pcd_path
    depth = 3
    m = la3dm_amd.BGKOctoMap(**dict(la3dm_amd.BGK_YAML, block_depth=depth), device=0)
    for i in (1, 2):
        xyz, origin = la3dm_amd.load_pcd(pcd_path("sim_structured", i))
        m.insert_pointcloud(xyz, origin, 0.1, 0.5, 8.0)
    assert m.is_device_resident()
    out = {}
    for c in CONNECTIVITIES:
        g = m.frontier(R.recipe_lo(), R.RECIPE_DIMS, open=FREE_M, unknown=UNK_M | MISS_M, connectivity=c, min_neighbours=1,
                       fields=("index", "nbrs", "score"))
        out.update({f"{k}{c}": np.asarray(g[k]) for k in ("n", "index", "nbrs", "score")})
    np.savez(sys.argv[1], **out)
