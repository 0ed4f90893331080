#!/usr/bin/env python
"""bench.py — voxel-updates/s of the BGK predict+fuse hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W]

Workload (BASELINE.json configs[1]): BGKOctoMap, synthetic 200k-ray scan, 0.1 m resolution,
config/methods/bgkoctomap.yaml parameters (block_depth 3, sf2 1, ell 0.2, free_res 0.5,
ds_resolution = resolution, priors 0.001).  A "step" is one pass of the hot path over the
scan: la3dm_bgk_scan_device() on the packed scan already resident in HBM (x/ell prescale
kernel + bgk_predict_fuse kernel), i.e. every leaf of every test block receives its fused
(ybar, kbar) from its <= 7 neighbour models and its alpha/beta/state update.
value = voxel-updates (leaves of test blocks) per second, whole job.

N > 1 (one process per GPU, launched by torch.distributed.run): weak scaling — every rank
owns one scan of the same size (different seed), runs the kernel on its blocks, and one RCCL
all-gather reassembles the updated (alpha, beta, state) grid of all ranks on every rank.  The leaf arrays
are double-buffered: the gather of scan k runs on RCCL's stream under the kernel of scan k + 1 (a buffer is
reused only after its gather has finished; all K kernels and all K gathers complete inside the timed region;
--no-overlap serialises them).

Adds to the JSON line: "roofline" (algorithmic bytes / HIP-event kernel time of the timed steps vs 8 TB/s).

A plain run sets up, warms up, times the K steps and prints the line, nothing else.  --full adds, at N=1, every
measurement that takes runs of its own: the other accumulate mode and the general kernel instance (roofline.ordered /
.double_sum, .general_instance), the out-of-cache and depth-4 legs, scale_n1, end_to_end, the gp / lv / bgkl legs and
"cpu_baseline" (the CPU oracle timed on the host cores on the same scan); the --no-* options leave parts of it out.

--dump-outputs DIR writes what the last timed step computed (the leaf alpha / beta / state arrays the hot path
updates; a map's leaves in --mode shard) as DIR/<name>.npy in float32, for comparing two builds output for output:
the inputs are seeded, so the same arguments give the same inputs on every run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

# multi-process GPU work on this pool needs dmabuf IPC (the image exports this already; keep it if the launcher drops it)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# the CPU legs run the restatement on every host core through OpenMP: its idle workers must sleep, not spin, or the host
# thread that drives the GPU in the legs that follow competes with 128 spinning threads (measured: the BGK-L insert 3.7 -> 11.5 ms)
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
os.environ.setdefault("GOMP_SPINCOUNT", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--fast-trig", type=int, default=0)
    ap.add_argument("--sum", type=int, default=-1, choices=[-1, 0, 1],
                    help="BGK accumulate mode: 0 = the reference's fp32 order (bit-identical), 1 = order-free double accumulators; -1 = default")
    ap.add_argument("--waves", type=int, default=0, help="waves per workgroup (kernel variant 3); 0 = library default")
    ap.add_argument("--remap", type=int, default=-1, help="workgroup->tile remap mode; -1 = library default")
    ap.add_argument("--workload", choices=["bgk", "gp", "lv", "l"], default="bgk",
                    help="bgk = BASELINE configs[1] (default, the contract line); gp = configs[2] (GPOctoMap, 50k rays); "
                         "lv = configs[3] (BGKLV, sim_unstructured scan, 0.05 m), l = BGKLOctoMap insert (row f4) — single-GPU side benches")
    ap.add_argument("--mode", choices=["hotpath", "shard", "scans"], default=None,
                    help="default: hotpath at N = 1 (the contract line: configs[1] through the hot-path kernel; it carries a `scale_n1` leg = "
                         "the shard workload on this one GPU), shard at N > 1.  `--gpus 1 --mode shard` runs the N > 1 workload at world = 1, "
                         "so that value(N) is ONE workload over N = 1, 2, 4, 8.  shard (strong scaling, BASELINE configs[4]): ONE 1M-ray scan at 0.05 m, every rank "
                         "holds a replica of the device-resident map, predicts + fuses its contiguous range of the test blocks, "
                         "one RCCL all-gather of the leaf payload (la3dm_devmap_set_shard); scans (weak scaling): one 200k-ray "
                         "scan per GPU through the hot-path kernel + an all-gather of its leaves (replicas)")
    ap.add_argument("--ablate", type=int, default=0, help="profiling only (results invalid): 1 skip k(r) evaluation, 2 skip tests")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N > 1: one leaf buffer, every all-gather finishes before the next kernel starts")
    ap.add_argument("--no-other-mode", action="store_true", help="skip the run of the other accumulate mode (roofline.ordered / .double_sum)")
    ap.add_argument("--no-side", action="store_true", help="skip the gp / lv / bgkl legs (BASELINE configs[2], configs[3], row f4)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end_to_end (device-resident insert_pointcloud) leg")
    ap.add_argument("--no-big", action="store_true",
                    help="skip the out-of-cache leg (configs[4]'s 1M-ray scan on this GPU: working set > the 256 MiB Infinity Cache)")
    ap.add_argument("--variants", action="store_true",
                    help="add roofline.kernel_function_variants: the headline launch with cheaper / no kernel-function evaluation (VERDICT r05 #2)")
    ap.add_argument("--no-cpu-omp", dest="cpu_omp", action="store_false",
                    help="skip the all-core OpenMP run of the oracle (cpu_baseline_omp)")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: add every measurement that takes runs of its own (other accumulate mode, general instance, "
                         "out-of-cache / depth-4 legs, scale_n1, end_to_end, gp / lv / bgkl legs, CPU baselines); the --no-* "
                         "options above and --variants apply to it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.variants and not args.full:
        ap.error("--variants: a leg of --full")
    if args.dump_outputs and args.workload != "bgk":
        ap.error("--dump-outputs: supported for --workload bgk only")

    import torch
    import la3dm_amd
    from la3dm_amd import _lib

    if args.workload != "bgk":
        return side_bench(args, torch, la3dm_amd, _lib)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback of the product path)")
    # LA3DM_BENCH_TEST_SINGLE_GPU=1: self-test of the N>1 code path on a 1-GPU box (all ranks on
    # cuda:0, gloo instead of RCCL, payload staged through host memory) — never a measurement.
    selftest = os.environ.get("LA3DM_BENCH_TEST_SINGLE_GPU") == "1"
    if selftest:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if selftest:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if args.mode is None:
        args.mode = "hotpath" if world == 1 else "shard"
    if args.mode == "hotpath" and world > 1:
        args.mode = "scans"      # (the hot-path kernel on N GPUs is the weak-scaling replica mode)
    if args.mode == "shard":     # (world = 1 too: the same workload on one unsharded map — the N = 1 point of the scaling series)
        return sharded_insert_bench(args, torch, dist, la3dm_amd, rank, world, local_rank, dev, selftest)

    # ---- build the workload (host side, untimed) -------------------------------------
    params = dict(la3dm_amd.BGK_YAML, resolution=args.resolution, block_depth=args.depth)
    shard_mode = False     # (N > 1 default mode returns above; what follows is N = 1 and --mode scans)
    xyz, origin = la3dm_amd.synthetic_scan(args.rays, seed=1234 + (0 if shard_mode else rank))
    m = la3dm_amd.BGKOctoMap(**params, device=local_rank)
    t0 = time.perf_counter()
    ok = m.prepare(xyz, origin, args.resolution, 0.5, -1.0)
    t_prepare = time.perf_counter() - t0
    assert ok
    st = m.stats()
    pk = m.packed()
    U = int(st["voxel_updates"])
    b_alg = 16 * int(st["train_reads"]) + 17 * U
    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # The leaf arrays live in ONE buffer laid out alpha | beta | state with room for the largest
    # rank, so the kernel's outputs are the all-gather payload (no packing copies).
    cap = pk.n_leaf
    if world > 1:
        cdev = torch.device("cpu") if selftest else dev
        n_leaf_max = torch.tensor([pk.n_leaf], device=cdev)
        dist.all_reduce(n_leaf_max, op=dist.ReduceOp.MAX)
        cap = int(n_leaf_max.item())
    cap = (cap + 63) // 64 * 64
    n = pk.n_leaf
    d = dict(train=up(pk.train_xyzy), train_off=up(pk.train_off.view(np.int32)), nbr=up(pk.nbr), center=up(pk.blk_center),
             leaf_off=up(pk.leaf_off.view(np.int32)), leaf_key=up(pk.leaf_key.view(np.int32)))
    # N > 1: two leaf buffers, so that the all-gather of scan k (RCCL's own stream) runs under the kernel of scan k + 1
    n_buf = 2 if (world > 1 and not args.no_overlap) else 1
    payloads, scans, keep = [], [], []
    for _ in range(n_buf):
        payload = torch.zeros(9 * cap, dtype=torch.uint8, device=dev)
        alpha_t = payload[0:4 * cap].view(torch.float32)[:n]
        beta_t = payload[4 * cap:8 * cap].view(torch.float32)[:n]
        state_t = payload[8 * cap:8 * cap + n]
        alpha_t.copy_(up(pk.alpha))
        beta_t.copy_(up(pk.beta))
        scan = _lib.BgkScan()
        scan.train_xyzy = d["train"].data_ptr()
        scan.train_off = d["train_off"].data_ptr()
        scan.n_train_pts = pk.n_train_pts
        scan.n_train_blk = pk.n_train_blk
        scan.nbr = d["nbr"].data_ptr()
        scan.blk_center = d["center"].data_ptr()
        scan.leaf_off = d["leaf_off"].data_ptr()
        scan.n_test_blk = pk.n_test_blk
        scan.n_leaf = pk.n_leaf
        scan.leaf_key = d["leaf_key"].data_ptr()
        scan.alpha = alpha_t.data_ptr()
        scan.beta = beta_t.data_ptr()
        scan.state = state_t.data_ptr()
        scan.flags = pk.flags          # LA3DM_SCAN_LABELS_01 from the front end (hits 1.0f, free samples 0.0f)
        payloads.append(payload)
        scans.append(scan)
        keep.append((alpha_t, beta_t, state_t))

    H = _lib.hip()
    ctx = m.ctx()
    if args.fast_trig:
        m.set_option("fast_trig", args.fast_trig)
    if args.waves:
        m.set_option("waves_per_wg", args.waves)
    if args.remap >= 0:
        m.set_option("remap", args.remap)
    if args.ablate:
        m.set_option("ablate", args.ablate)
    stream = torch.cuda.current_stream().cuda_stream

    gather_out = [torch.zeros(world * cap * 9, dtype=torch.uint8, device=dev) for _ in range(n_buf)] if world > 1 else None
    pending = [None] * n_buf
    counter = [0]

    def step():
        b = counter[0] % n_buf
        counter[0] += 1
        if pending[b] is not None:       # the gather that still reads this buffer (two scans ago)
            pending[b].wait()
            pending[b] = None
        rc = H.la3dm_bgk_scan_device(ctx, C.byref(scans[b]), stream, None)
        if rc != 0:
            raise RuntimeError(H.la3dm_last_error(ctx).decode())
        if world > 1:
            if selftest:
                host = torch.zeros(world * cap * 9, dtype=torch.uint8)
                dist.all_gather_into_tensor(host, payloads[b].cpu())
                gather_out[b].copy_(host)
            elif n_buf > 1:
                pending[b] = dist.all_gather_into_tensor(gather_out[b], payloads[b], async_op=True)
            else:
                dist.all_gather_into_tensor(gather_out[b], payloads[b])

    def sync():
        for b in range(n_buf):
            if pending[b] is not None:
                pending[b].wait()
                pending[b] = None
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def timed(steps):
        for _ in range(args.warmup):
            step()
        m.set_option("time_kernel", 1)
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        dt_ = time.perf_counter() - t0
        kt = np.zeros(steps + 8, np.float32)
        nk = C.c_uint32()
        H.la3dm_kernel_times(ctx, kt.ctypes.data, kt.size, C.byref(nk))
        m.set_option("time_kernel", 0)
        return dt_, (float(kt[:nk.value].mean()) if nk.value else float("nan"))

    def restore_leaves():
        # the steps update the leaves in place: back to the scan's own leaves, so that what the timed steps compute
        # (--dump-outputs) depends on --warmup and --steps only
        torch.cuda.synchronize()
        for alpha_t, beta_t, state_t in keep:
            alpha_t.copy_(up(pk.alpha))
            beta_t.copy_(up(pk.beta))
            state_t.zero_()

    sum_mode = args.sum if args.sum >= 0 else int(os.environ.get("LA3DM_BGK_SUM", "1"))
    if world == 1:
        # bring the GPU to steady state before anything is timed (>= 100 launches and >= 0.2 s of them): --warmup's few
        # launches of a < 0.1 ms step do not (configs[1], --warmup 5: 0.080 ms per step after them alone, 0.072 after this)
        m.set_option("bgk_sum", sum_mode)
        t0, n_settle = time.perf_counter(), 0
        while n_settle < 100 or time.perf_counter() - t0 < 0.2:
            for _ in range(10):
                step()
            n_settle += 10
            torch.cuda.synchronize()
        restore_leaves()
    # the other accumulate mode first (N = 1 only, its own short run), then the mode the line is quoted on
    other = None
    if args.full and world == 1 and not args.no_other_mode:
        m.set_option("bgk_sum", 1 - sum_mode)
        dt_o, k_o = timed(min(args.steps, 20))
        other = {"bgk_sum": 1 - sum_mode, "ms_per_step": dt_o / min(args.steps, 20) * 1e3, "kernel_ms": k_o}
    m.set_option("bgk_sum", sum_mode)
    # the same launch without LA3DM_SCAN_FULL_BLOCKS (what a scan into a map with pruned blocks runs: the instance that
    # carries the general path beside the table path) — its own short run, quoted next to the headline
    general = None
    if args.full and world == 1 and sum_mode == 1 and not args.no_other_mode and (scans[0].flags & 4):
        for sc in scans:
            sc.flags &= ~4
        _, k_g = timed(min(args.steps, 20))
        for sc in scans:
            sc.flags |= 4
        general = {"kernel_ms": k_g, "what": "the same scan without LA3DM_SCAN_FULL_BLOCKS: the kernel instance with the general (pruned-block) path compiled in"}
    if other or general:
        restore_leaves()
    dt, k_ms = timed(args.steps)
    if args.dump_outputs and rank == 0:
        # the buffer the last timed step wrote (this rank's own leaves)
        alpha_t, beta_t, state_t = keep[(counter[0] - 1) % n_buf]
        dump_outputs(args.dump_outputs, {"alpha": alpha_t.cpu().numpy(), "beta": beta_t.cpu().numpy(),
                                         "state": state_t.cpu().numpy()})

    total_U = U
    if world > 1:
        cdev = torch.device("cpu") if selftest else dev
        tt = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        uu = torch.tensor([U], dtype=torch.float64, device=cdev)
        dist.all_reduce(uu, op=dist.ReduceOp.SUM)
        total_U = int(uu.item())

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = total_U / (dt / args.steps)
        achieved = b_alg / (k_ms * 1e-3) / 1e9
        counters = profiled_counters(f"rays{args.rays}_d{args.depth}_r{args.resolution}_sum{sum_mode}")
        traffic = counters.get("hbm_bytes_per_launch") if counters else None
        out = {
            "metric": "voxel-updates/sec per scan (200k pts, 0.1 m res); HBM GB/s vs roofline",
            "value": value, "unit": "voxel-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "none" if world == 1 else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BGKOctoMap synthetic {args.rays}-ray scan, {args.resolution} m res, "
                                   f"block_depth {args.depth}, bgkoctomap.yaml kernel params (configs[1])",
                       "rays": args.rays, "resolution": args.resolution, "block_depth": args.depth,
                       "ds_resolution": args.resolution, "free_resolution": 0.5,
                       "hits": int(st["n_hits"]), "frees": int(st["n_frees"]),
                       "test_blocks": int(st["n_test_blocks"]), "train_blocks": int(st["n_train_blocks"]),
                       "voxel_updates_per_scan": U, "pair_evals_per_scan": int(st["pair_evals"]),
                       "parallelism": ("single GPU" if world == 1 else
                                       "1 scan per GPU + RCCL all-gather of leaf (alpha,beta,state)") +
                                      (", gather of scan k under the kernel of scan k+1 (two leaf buffers)" if n_buf > 1 else ""),
                       "trig": ["correctly-rounded", "f32-poly", "ocml"][args.fast_trig],
                       "accumulate": ACC_NAMES[sum_mode], "bgk_sum": sum_mode, "waves_per_wg": args.waves, "remap": args.remap},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                         "frac": achieved / 8000.0, "traffic": traffic,
                         "kernel": kernel_name(m, sum_mode, scans[0].flags, pk), "kernel_ms": k_ms, "algorithmic_bytes_per_launch": b_alg,
                         "pair_evals_per_s": int(st["pair_evals"]) / (k_ms * 1e-3)},
            "host": {"prepare_s": t_prepare, "frontend_s": st["t_frontend"], "partition_s": st["t_partition"],
                     "pack_s": st["t_pack"]},
        }
        if other:
            ach_o = b_alg / (other["kernel_ms"] * 1e-3) / 1e9
            out["roofline"]["ordered" if other["bgk_sum"] == 0 else "double_sum"] = dict(
                other, accumulate=ACC_NAMES[other["bgk_sum"]], kernel=kernel_name(m, other["bgk_sum"], scans[0].flags, pk), achieved=ach_o,
                frac=ach_o / 8000.0, voxel_updates_per_s=U / (other["ms_per_step"] * 1e-3))
        if general:
            ach_g = b_alg / (general["kernel_ms"] * 1e-3) / 1e9
            out["roofline"]["general_instance"] = dict(general, kernel=kernel_name(m, sum_mode, scans[0].flags & ~4, pk), achieved=ach_g, frac=ach_g / 8000.0)
        if counters:
            # Instruction-issue roofline (the kernel is issue bound, not HBM bound).  Peaks are MEASURED on this chip
            # (profiles/r02/valu_issue.txt, tools/ubench/valu_issue.hip): a SIMD issues one instruction of any kind per
            # 2.2 cycles at best, and most VALU instructions of this kernel's mix occupy it for 4.1 cycles.
            n_valu, n_salu, n_lds = (counters.get(k, 0) for k in ("valu_insts_per_launch", "salu_insts_per_launch", "lds_insts_per_launch"))
            simds, clk = 1024, 2.4e9
            rate = (n_valu + n_salu + n_lds) / (k_ms * 1e-3)
            out["roofline"]["issue"] = {
                "achieved": rate, "peak": simds * clk / 2.2, "unit": "wave-instr/s (VALU+SALU+LDS)",
                "frac": rate / (simds * clk / 2.2), "valu_insts_per_launch": n_valu, "salu_insts_per_launch": n_salu,
                "lds_insts_per_launch": n_lds,
                "valu_only": {"achieved": n_valu / (k_ms * 1e-3), "peak_fast_class": simds * clk / 2.2,
                              "peak_4cycle_class": simds * clk / 4.1},
                "source": counters.get("source")}
        else:
            out["roofline"]["traffic_note"] = ("profiles/bgk_traffic.json has no entry stamped with this build's kernel source "
                                               "hash for this workload: counters omitted (tools/prof/update_traffic.sh regenerates)")
        if args.full and world == 1 and not shard_mode and not args.no_e2e:
            out["end_to_end"] = end_to_end(la3dm_amd, params, args)
        if args.full and world == 1 and not args.no_big and args.rays == 200000:
            out["roofline"]["out_of_cache"] = out_of_cache_leg(la3dm_amd, _lib, torch, dev)
            out["roofline"]["depth4"] = depth4_leg(la3dm_amd, _lib, torch, dev)
            if args.variants:
                out["roofline"]["kernel_function_variants"] = kernel_variants_leg(la3dm_amd, _lib, torch, dev)
            # the N = 1 point of the multi-GPU series (`--gpus N` times configs[4]'s whole insert, not this line's kernel-only step):
            # the same W + K inserts `--gpus N --mode shard` runs, on this GPU — equals that line's `single_gpu`
            out["scale_n1"] = scale_n1_leg(la3dm_amd, torch, dev, args)
        if args.full and world == 1 and not args.no_side:
            # the other BASELINE configs on this GPU, each with its own roofline and CPU leg (same protocol as --workload X);
            # every GPU measurement of the run comes before the first all-core CPU leg
            del m
            torch.cuda.synchronize()
            side = argparse.Namespace(**vars(args))
            side.steps, side.warmup = 10, 2
            # (GP depth 4 last: it frees gigabytes of factor arenas when it ends, see l_leg)
            out["bgkl"] = l_leg(side, torch, la3dm_amd, cpu=False)
            out["lv"] = lv_leg(side, torch, la3dm_amd, _lib, cpu=False)
            out["gp"] = {"depth3": gp_leg(side, torch, la3dm_amd, _lib, depth=3, cpu=False)}
            out["gp"]["depth4"] = gp_leg(side, torch, la3dm_amd, _lib, depth=4, cpu=False)
        if args.full and world == 1 and not args.no_cpu:
            out["cpu_baseline"] = cpu_baseline(params, xyz, origin, args, U)
            if args.cpu_omp:
                out["cpu_baseline_omp"] = cpu_baseline(params, xyz, origin, args, U, omp=True)
            if not args.no_side:
                out["gp"]["depth3"]["cpu_baseline"] = gp_cpu(la3dm_amd)
                if args.cpu_omp:   # (a bounded sample: one quadrant of the scan)
                    out["gp"]["depth4"]["cpu_baseline"] = gp_cpu(la3dm_amd, depth=4)
                out["lv"]["cpu_baseline"] = lv_cpu(la3dm_amd, out["lv"])
                if args.cpu_omp:
                    out["lv"]["cpu_baseline_omp"] = lv_cpu(la3dm_amd, out["lv"], omp=True)
                out["bgkl"]["cpu_baseline"] = l_cpu(la3dm_amd)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


ACC_SIDE = {0: "the reference's fp32 running sums in row / gather order (bit-identical to the CPU restatement)",
            1: "double sums of the same fp32 terms, rounded once per neighbour (BGK-L) / voxel (BGK-LV) — library default since round 5"}
ACC_NAMES = {0: "the reference's fp32 summation order (bit-identical to the CPU restatement)",
             1: "double accumulators per leaf, alpha / beta rounded once (library default; |dp| <= ~4e-7 from the reference order)"}


DUMP_MAX_BYTES = 60 * 10 ** 6      # array data of one dump: with the .npy headers, under 64 MB in all


def dump_outputs(path, arrays):
    """--dump-outputs: each array (all of one length, one entry per leaf) as <path>/<name>.npy in float32.  Above
    DUMP_MAX_BYTES in all, the same fixed, seeded sample of the leaves from every array, its indices in
    sample_index.npy (float64)."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v).astype(np.float32) for k, v in arrays.items()}
    n = len(next(iter(arrays.values())))
    assert all(len(v) == n for v in arrays.values())
    if 4 * len(arrays) * n > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (4 * len(arrays) + 8)
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["sample_index"] = idx.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), np.ascontiguousarray(v))


def kernel_name(m, sum_mode, flags, pk):
    """the predict + fuse kernel la3dm_bgk_scan_device launches for these options and scan flags (la3dm_hip.hip), with its
    template arguments <fast_trig, general path compiled in>"""
    if sum_mode == 0:
        return "bgk_predict_fuse_v5"
    trig = m.get_option("fast_trig")
    if not (m.get_option("bgk_tables") and (flags & 2)):
        return f"bgk_predict_fuse_r<{trig}>"
    full = bool(flags & 4) and int(pk.n_leaf) == int(pk.n_test_blk) * 8 ** (int(m.block_depth) - 1)
    return f"bgk_predict_fuse_t<{trig}, {'false' if full else 'true'}>"


def shard_workload(args):
    """configs[4]: the 1M-ray scan at 0.05 m (or what --rays / --resolution ask for)"""
    return (1000000, 0.05) if args.rays == 200000 else (args.rays, args.resolution)


def insert_loop(m, torch, d_cloud, origin, res, steps, warm, barrier=None):
    """W untimed + K timed device-resident insert_pointcloud calls of the cloud in HBM -> (seconds, voxel updates of the K steps)"""
    def fence():
        torch.cuda.synchronize()
        if barrier is not None:
            barrier()
            torch.cuda.synchronize()
    ups = 0
    for _ in range(warm):
        m.insert_pointcloud_device(d_cloud.data_ptr(), d_cloud.shape[0], origin, res, 0.5, -1.0)
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.insert_pointcloud_device(d_cloud.data_ptr(), d_cloud.shape[0], origin, res, 0.5, -1.0)
        ups += int(m.stats()["voxel_updates"])
    fence()
    return time.perf_counter() - t0, ups


def scale_n1_leg(la3dm_amd, torch, dev, args):
    rays, res = shard_workload(args)
    params = dict(la3dm_amd.BGK_YAML, resolution=res, block_depth=args.depth)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    d_cloud = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev)
    m = la3dm_amd.BGKOctoMap(**params, device=dev.index or 0)
    steps = min(args.steps, 20)
    dt, ups = insert_loop(m, torch, d_cloud, origin, res, steps, min(args.warmup, 3))
    del m
    return {"what": f"BGKOctoMap synthetic {rays}-ray scan, {res} m res (configs[4]); a step = one whole device-resident insert_pointcloud, cloud "
                    "in HBM, re-inserted every step: the workload of `--gpus N` (N > 1) and of `--gpus 1 --mode shard`, on this one GPU",
            "value": ups / dt, "unit": "voxel-updates/s", "ms_per_step": dt / steps * 1e3, "steps": steps}


def sharded_insert_bench(args, torch, dist, la3dm_amd, rank, world, local_rank, dev, selftest):
    """`--mode shard` (N > 1 default): BASELINE configs[4] — ONE synthetic 1M-ray scan at 0.05 m, block-sharded.  Every rank holds a
    replica of the device-resident map and is handed the same cloud (resident in its HBM); a step is one whole
    BGKOctoMap::insert_pointcloud: front end + partition redundantly on every GPU, predict + fuse of the rank's contiguous
    range of test blocks, ONE all-gather of the leaf payload over RCCL, commit + prune everywhere.  Strong scaling: the
    work per step is fixed, value = voxel updates of the timed steps / max-over-ranks time.  world = 1 (`--gpus 1 --mode shard`)
    is the same workload on one unsharded map, so value(N) is one workload for every N.  Every rank also times the same
    steps unsharded on its own GPU beforehand so the line carries its own single-GPU reference."""
    from la3dm_amd import sharding
    rays, res = shard_workload(args)
    params = dict(la3dm_amd.BGK_YAML, resolution=res, block_depth=args.depth)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    d_cloud = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev)
    cdev = torch.device("cpu") if selftest else dev
    barrier = dist.barrier if dist is not None else None

    def callback():
        return sharding.torch_allgather(dist, rank, dev, stage_through_host=selftest)

    # single-GPU reference: the same W + K inserts on an unsharded replica (all ranks do it, so every GPU is equally warm)
    ref = la3dm_amd.BGKOctoMap(**params, device=local_rank)
    dt1, ups1 = insert_loop(ref, torch, d_cloud, origin, res, args.steps, args.warmup, barrier)
    del ref
    m = la3dm_amd.BGKOctoMap(**params, device=local_rank)
    if world > 1:
        m.set_shard(rank, world, callback())
    m.set_option("time_kernel", 1)       # HIP events around the predict + fuse kernel of every insert (this rank's range)
    dt, ups = insert_loop(m, torch, d_cloud, origin, res, args.steps, args.warmup, barrier)
    from la3dm_amd import _lib
    kt = np.zeros(args.steps + args.warmup + 8, np.float32)
    nk = C.c_uint32()
    _lib.hip().la3dm_kernel_times(m.ctx(), kt.ctypes.data, kt.size, C.byref(nk))
    k_ms = float(kt[max(0, nk.value - args.steps):nk.value].mean()) if nk.value else float("nan")
    if args.dump_outputs and rank == 0:
        lv = m.leaves()        # the map after the last timed insert (a replica: the same on every rank)
        dump_outputs(args.dump_outputs, {"A": lv["A"], "B": lv["B"], "state": lv["state"]})
    if world > 1:
        tt = torch.tensor([dt, dt1], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt, dt1 = float(tt[0].item()), float(tt[1].item())
    st = m.stats()
    # per-stage wall times of EVERY rank (a third replica created with LA3DM_TIMING=1: a host synchronisation after every stage,
    # so the sum is larger than an untimed step — it says where the time goes and how even the ranks are, not how long a step takes)
    os.environ["LA3DM_TIMING"] = "1"
    try:
        mt = la3dm_amd.BGKOctoMap(**params, device=local_rank)
    finally:
        os.environ.pop("LA3DM_TIMING", None)
    if world > 1:
        mt.set_shard(rank, world, callback())
    stages = {}
    for i in range(3):
        mt.insert_pointcloud_device(d_cloud.data_ptr(), d_cloud.shape[0], origin, res, 0.5, -1.0)
        sx = mt.stats()
        stages = {"front_end": sx["t_frontend"] * 1e3, "partition": sx["t_partition"] * 1e3, "test_list_blocks_leaves": sx["t_pack"] * 1e3,
                  "predict_fuse_own_range": sx["t_device"] * 1e3, "allgather_v": sx["t_gather"] * 1e3,
                  "commit_prune": sx["t_commit"] * 1e3, "predict_fuse_kernel_events_ms": k_ms}
    torch.cuda.synchronize()
    all_stages = [stages]
    if world > 1:
        dist.barrier()
        all_stages = [None] * world
        dist.all_gather_object(all_stages, stages)
    del mt
    if rank == 0:
        b_alg = 16 * int(st["train_reads"]) + 17 * int(st["voxel_updates"])
        print(json.dumps({
            "metric": "voxel-updates/sec per scan (200k pts, 0.1 m res); HBM GB/s vs roofline",
            "value": ups / dt, "unit": "voxel-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BGKOctoMap synthetic {rays}-ray scan, {res} m res, block_depth {args.depth}, bgkoctomap.yaml "
                                   "kernel params (configs[4]); a step = one device-resident insert_pointcloud of the scan "
                                   "(re-inserted every step), cloud resident in HBM",
                       "rays": rays, "resolution": res, "block_depth": args.depth,
                       "parallelism": ("one GPU, unsharded map (the N = 1 point of the `--mode shard` series)" if world == 1 else
                                       f"block-sharded over {world} GPUs: replicated map, contiguous equal-weight ranges of the "
                                       "test blocks per rank, a rank lists the leaves of its own range only, one in-place all-gather-v of the "
                                       "leaves' (alpha, beta, state, key) per insert queued on the map's stream (13 B per leaf, no padding, no "
                                       "host synchronisation); x-slab partition (per-block counts global, membership pairs / sort / CSR / rows per rank for its own slab); "
                                       "front end (but the sample filter), leaf count, commit + prune redundant on every rank"),
                       "voxel_updates_last_step": int(st["voxel_updates"]), "test_blocks": int(st["n_test_blocks"]),
                       "allgather_v_bytes_total": 13 * int(st["voxel_updates"]) if world > 1 else 0,
                       "process_group": None if dist is None else
                                        {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                                         "exchange": os.environ.get("LA3DM_SHARD_EXCHANGE", "p2p") + " (sharding.exchange_v: one grouped batch of sends / receives per exchange; LA3DM_SHARD_EXCHANGE=broadcast: one broadcast per rank and array)"}},
            "stages_ms_rank0": stages,
            "stages_ms_by_rank": all_stages,
            "roofline": {"bound": "hbm", "achieved": b_alg / world / (k_ms * 1e-3) / 1e9,
                         "peak": 8000.0, "unit": "GB/s",
                         "frac": b_alg / world / (k_ms * 1e-3) / 1e9 / 8000.0,
                         "traffic": None, "kernel": "bgk_predict_fuse (rank 0's range of the last steps; algorithmic bytes of the "
                                                    "scan / world: the ranges are cut to equal weight)", "kernel_ms": k_ms},
            "single_gpu": {"what": "the same steps on one unsharded replica, measured in this run on every rank's own GPU (max)",
                           "value": ups1 / dt1, "ms_per_step": dt1 / args.steps * 1e3},
            "speedup_vs_single_gpu": (ups / dt) / (ups1 / dt1)}))
    if dist is not None:
        dist.destroy_process_group()


def kernel_source_files(sources=("bgk_kernels.h",)):
    """the files a kernel is built from: the named sources of la3dm_amd/csrc plus everything they #include "locally",
    transitively (bgk_kernels.h -> sincos_table.inc; gp_kernels.h / lv_kernels.h -> bgk_kernels.h -> ...), in a fixed order"""
    import re
    base = os.path.join(ROOT, "la3dm_amd", "csrc")
    seen, order, todo = set(), [], list(sources)
    while todo:
        f = todo.pop(0)
        if f in seen:
            continue
        seen.add(f)
        order.append(f)
        with open(os.path.join(base, f), "r", errors="replace") as fh:
            incs = re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), flags=re.M)
        todo.extend(i for i in incs if os.path.exists(os.path.join(base, i)))
    return order


def kernel_source_hash(sources=("bgk_kernels.h",)):
    """sha256 over kernel_source_files(sources) (the launch side is covered by the waves-per-launch check in
    profiled_counters): PMC numbers quoted from profiles/ are only valid for this kernel.
    tests/test_profiles_stamps_cpu.py fails while any entry of profiles/*.json carries another hash."""
    import hashlib
    h = hashlib.sha256()
    for f in kernel_source_files(sources):
        with open(os.path.join(ROOT, "la3dm_amd", "csrc", f), "rb") as fh:
            h.update(f.encode() + b"\0")
            h.update(fh.read())
    return h.hexdigest()[:16]


# which sources each stamped counter file's entries are recorded against (bench legs, tools/prof/*.sh and
# tests/test_profiles_stamps_cpu.py all read this table)
STAMPED = {
    "bgk_traffic.json": {None: ("bgk_kernels.h",)},
    "gp_counters.json": {None: ("gp_kernels.h",)},
    "side_counters.json": {"lv50k": ("lv_kernels.h", "devmap_lv_kernels.h"), "lvseq": ("lv_kernels.h", "devmap_lv_kernels.h"),
                           "l": ("bgkl_kernels.h",)},
}


def stamped_sources(path, key):
    t = STAMPED[path]
    return t.get(key, t.get(None))


def profiled_counters(key, tiles=None, path="bgk_traffic.json", sources=("bgk_kernels.h",)):
    """per-launch PMC counters of the dominant kernel for this workload, from profiles/<path> — refused unless the entry
    was recorded with the kernel source this build was made from (tools/prof/update_traffic.sh stamps it) and, when the
    caller knows it, with the number of waves this run launches"""
    tpath = os.path.join(ROOT, "profiles", path)
    try:
        with open(tpath) as f:
            e = json.load(f).get(key)
    except Exception:
        return None
    if not e or e.get("kernel_sha") != kernel_source_hash(sources):
        return None
    if tiles is not None and e.get("waves_per_launch") is not None and int(e["waves_per_launch"]) != int(tiles):
        return None
    return e


def _upload(torch, dev, keep):
    def up(ptr, nbytes):
        if not ptr or nbytes == 0:
            return 0
        buf = (C.c_char * nbytes).from_address(ptr)
        t = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        keep.append(t)
        return t.data_ptr()
    return up


def _time_calls(torch, H, m, call, steps, warmup):
    for _ in range(warmup):
        assert call() == 0, H.la3dm_last_error(m.ctx())
    m.set_option("time_kernel", 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        assert call() == 0
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    kt = np.zeros(steps + 8, np.float32)
    nk = C.c_uint32()
    H.la3dm_kernel_times(m.ctx(), kt.ctypes.data, kt.size, C.byref(nk))
    m.set_option("time_kernel", 0)
    return dt, float(kt[:nk.value].mean())


def gp_leg(args, torch, la3dm_amd, _lib, depth, cpu):
    """BASELINE configs[2]: GPOctoMap, synthetic 50 000-ray scan, 0.1 m, gpoctomap.yaml (block_depth 3; depth 4 = the
    constructor default, where blocks hold hundreds of points and the solve runs on the matrix cores).  A step =
    la3dm_gp_scan_device on the packed scan resident in HBM: Cholesky + alpha per training block, predict + fuse."""
    dev = torch.device("cuda", 0)
    H = _lib.hip()
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    up = _upload(torch, dev, keep)
    rays = 50000
    params = dict(la3dm_amd.GP_YAML, block_depth=depth, resolution=0.1)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    m = la3dm_amd.GPOctoMap(**params, device=0)
    assert m.prepare(xyz, origin, 0.1, 0.1, -1.0)
    st, pk = m.stats(), m.packed()
    c = pk.c
    scan = _lib.BgkScan()
    for f, n in (("train_xyzy", 16 * c.n_train_pts), ("train_off", 4 * (c.n_train_blk + 1)), ("nbr", 28 * c.n_test_blk),
                 ("blk_center", 12 * c.n_test_blk), ("leaf_off", 4 * (c.n_test_blk + 1)), ("leaf_key", 4 * c.n_leaf),
                 ("alpha", 4 * c.n_leaf), ("beta", 4 * c.n_leaf), ("state", c.n_leaf)):
        setattr(scan, f, up(getattr(c, f), n))
    for f in ("n_train_pts", "n_train_blk", "n_test_blk", "n_leaf", "flags", "train_max_n", "train_sum_n2"):
        setattr(scan, f, getattr(c, f))
    nb = np.diff(pk.train_off.astype(np.int64))
    nbr = np.asarray(pk.nbr).reshape(-1, 7)
    nleaf = np.diff(pk.leaf_off.astype(np.int64))
    nn = np.where(nbr >= 0, nb[np.maximum(nbr, 0)], 0).astype(np.float64)
    flops = float((nleaf[:, None] * (nn ** 2 + 4 * nn)).sum())      # per leaf and neighbour: N^2 (v = L^-1 Ks) + 4 N (Ks, m)
    dt, k_ms = _time_calls(torch, H, m, lambda: H.la3dm_gp_scan_device(m.ctx(), C.byref(scan), stream, None), args.steps, args.warmup)
    U = int(st["voxel_updates"])
    out = {"workload": f"GPOctoMap synthetic {rays}-ray scan, 0.1 m, block_depth {depth}, gpoctomap.yaml (configs[2]"
                       + (")" if depth == 3 else "; block_depth 4 = constructor default)"),
           "ms_per_step": dt * 1e3, "voxel_updates_per_s": U / dt, "voxel_updates_per_scan": U,
           "steps": args.steps, "steps_include": "gp_train (Cholesky + alpha per training block) + gp_predict_fuse",
           "max_N": int(c.train_max_n), "train_blocks": int(c.n_train_blk), "test_blocks": int(c.n_test_blk),
           "flops_per_step": flops,
           "roofline": {"bound": "mfma", "kernel": "gp_predict_fuse (small + large launches)", "kernel_ms": k_ms,
                        "achieved": flops / 1e12 / (k_ms * 1e-3), "peak": 157.3, "unit": "TFLOP/s",
                        "frac": flops / 1e12 / (k_ms * 1e-3) / 157.3,
                        "note": "fp32 MFMA peak; blocks with N <= 64 (all of depth 3 but a few) run the VALU forward "
                                "substitution, see valu_issue"}}
    cnt = profiled_counters(f"gp_rays{rays}_d{depth}", path="gp_counters.json", sources=("gp_kernels.h",))
    if cnt:
        rate = (cnt["valu_insts_per_launch"] + cnt["salu_insts_per_launch"] + cnt["lds_insts_per_launch"]) / (k_ms * 1e-3)
        out["roofline"]["valu_issue"] = {"achieved": cnt["valu_insts_per_launch"] / (k_ms * 1e-3), "peak": 1024 * 2.4e9 / 4.0,
                                         "unit": "VALU wave-instr/s (one per 4 cycles per SIMD)",
                                         "frac": cnt["valu_insts_per_launch"] / (k_ms * 1e-3) / (1024 * 2.4e9 / 4.0),
                                         "all_insts_per_s": rate, "source": cnt.get("source")}
    if depth == 3:
        # the same step in option "gp_mode" 1 (gp_eigen_kernels.h): the order of an SSE2 build of Eigen 3.3.7 — no FMA, packet sums, panelled
        # solves, fp32 pexp — bit-identical to the restatement's set_gp_mode(1) (reported next to mode 0, which stays the default)
        m.set_option("gp_mode", 1)
        dt1, k1 = _time_calls(torch, H, m, lambda: H.la3dm_gp_scan_device(m.ctx(), C.byref(scan), stream, None), args.steps, args.warmup)
        m.set_option("gp_mode", 0)
        out["gp_mode_1"] = {"what": "Eigen 3.3.7 / SSE2 order of operations on the VALU (no FMA, 4-lane packet sums, llt_inplace blocking, panels of 8 "
                                    "with reciprocal diagonals, packet exp); an option, the default is gp_mode 0",
                            "ms_per_step": dt1 * 1e3, "kernel_ms": k1, "voxel_updates_per_s": U / dt1}
    if cpu:
        out["cpu_baseline"] = gp_cpu(la3dm_amd, depth=depth)
    del m
    return out


def gp_cpu(la3dm_amd, depth=3):
    """CPU leg of the GP legs: the OpenMP build of the restatement on the full scan (depth 3), or — depth 4, where one
    insert is ~1.4 Tflop of scalar fp32 — on a BOUNDED sample of it: the rays of one quadrant around the sensor (same
    point density, hence the same block sizes up to N ~ 500; a quarter of the blocks)"""
    from oracle import oracle as O
    params = dict(la3dm_amd.GP_YAML, block_depth=depth, resolution=0.1)
    xyz, origin = la3dm_amd.synthetic_scan(50000)
    sample = "the full scan"
    if depth >= 4:
        d = xyz - np.asarray(origin, np.float32)[None, :]
        xyz = np.ascontiguousarray(xyz[(d[:, 0] >= 0) & (d[:, 1] >= 0)])
        sample = f"the {xyz.shape[0]} rays of the scan's +x +y quadrant"
    o = O.OracleGPMap(**params, omp=True)
    t0 = time.perf_counter()
    o.insert_pointcloud(xyz, origin, 0.1, 0.1, -1.0)
    tc = time.perf_counter() - t0
    so = o.stats()
    return {"value": so["voxel_updates"] / so["t_predict"], "unit": "voxel-updates/s",
            "cores": O.lib(True).orc_num_threads(), "kind": "port",
            "sample": f"{sample} at block_depth {depth}, 1 insert_pointcloud into a fresh map of this repo's restatement (OpenMP "
                      "build); value = leaves of test blocks / train+predict+fuse stage time",
            "voxel_updates": so["voxel_updates"], "stage_s": {"predict_fuse": so["t_predict"], "insert_pointcloud": tc}}


def lv_leg(args, torch, la3dm_amd, _lib, cpu):
    """BASELINE configs[3]: BGKLVOctoMap, the 12 sim_unstructured scans at 0.05 m (bgklvoctomap.yaml, block_depth 5,
    max_range 8) fused into one device-resident map, one insert_pointcloud per scan; plus a synthetic 50 000-ray scan
    at the same parameters (a workload that fills the GPU)."""
    H = _lib.hip()
    params = dict(la3dm_amd.LV_YAML, resolution=0.05, block_depth=5)
    scans = [la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_unstructured", f"sim_unstructured_{i}.pcd"))
             for i in range(1, 13)]

    def sequence():
        m = la3dm_amd.BGKLVOctoMap(**params, device=0)
        m.set_option("time_kernel", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for xyz, origin in scans:
            m.insert_pointcloud(xyz, origin, 0.05, 0.1, 8.0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kt = np.zeros(256, np.float32)
        nk = C.c_uint32()
        H.la3dm_kernel_times(m.ctx(), kt.ctypes.data, kt.size, C.byref(nk))
        return dt, float(kt[:nk.value].sum()), int(nk.value), m
    sequence()                                   # library warm-up (arena growth)
    runs = [sequence()[:3] for _ in range(3)]
    dt, ksum, nk = sorted(runs)[1]
    out = {"workload": "BGKLVOctoMap, the 12 sim_unstructured scans fused, 0.05 m, block_depth 5, bgklvoctomap.yaml, max_range 8 "
                       "(configs[3]); a step = the whole 12-scan sequence into a fresh device-resident map (host clouds)",
           "sequence_ms": dt * 1e3, "ms_per_scan": dt * 1e3 / 12, "voxel_kernel_ms_sum": ksum, "voxel_kernel_launches": nk,
           "points_per_scan": int(np.mean([x.shape[0] for x, _ in scans]))}
    # a scan that fills the GPU: synthetic 50 000 rays, same parameters
    xyz, origin = la3dm_amd.synthetic_scan(50000)
    m = la3dm_amd.BGKLVOctoMap(**params, device=0)
    m.insert_pointcloud(xyz, origin, 0.05, 0.1, 8.0)
    m.set_option("time_kernel", 1)
    each = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.insert_pointcloud(xyz, origin, 0.05, 0.1, 8.0)
        torch.cuda.synchronize()
        each.append(time.perf_counter() - t0)
    dt_b = float(np.median(each))   # (median: see l_leg)
    kt = np.zeros(64, np.float32)
    nk2 = C.c_uint32()
    H.la3dm_kernel_times(m.ctx(), kt.ctypes.data, kt.size, C.byref(nk2))
    st = m.lv_stats()
    k_ms = float(kt[:nk2.value].sum()) / 3
    b_alg = 16 * int(st["n_samples"]) + 9 * int(st["voxels"])
    out["synthetic_50k"] = {"workload": "BGKLVOctoMap synthetic 50000-ray scan re-inserted, 0.05 m, block_depth 5, max_range 8",
                            "ms_per_insert": dt_b * 1e3, "samples": int(st["n_samples"]), "voxels": int(st["voxels"]),
                            "accumulate": ACC_SIDE[m.get_option("bgk_sum")],
                            "roofline": {"bound": "hbm", "kernel": "bgklv_voxel_kernel_w8 (+ bgklv_split_apply64)" if m.get_option("bgk_sum") == 1
                                         else "bgklv_voxel_kernel<false> (+ bgklv_split_add_kernel)", "kernel_ms": k_ms,
                                         "algorithmic_bytes_per_launch": b_alg, "achieved": b_alg / (k_ms * 1e-3) / 1e9,
                                         "peak": 8000.0, "unit": "GB/s", "frac": b_alg / (k_ms * 1e-3) / 1e9 / 8000.0}}
    cnt = profiled_counters("lv50k", path="side_counters.json", sources=("lv_kernels.h", "devmap_lv_kernels.h"))
    if cnt:   # HBM bytes per insert of the kernels the roofline names (tools/prof/side_pmc.sh; gfx950: FETCH_SIZE x 2 + WRITE_SIZE)
        ks = [e for k, e in cnt["kernels"].items() if "bgklv_voxel_kernel" in k or "bgklv_split_a" in k]
        rf = out["synthetic_50k"]["roofline"]
        rf["traffic"] = sum((2 * e.get("FETCH_SIZE", 0.0) + e.get("WRITE_SIZE", 0.0)) * 1024 for e in ks)
        rf["traffic_source"] = cnt.get("source")
        rf["valu_insts"] = sum(e.get("SQ_INSTS_VALU", 0.0) for e in ks)
        rf["insert_traffic_all_kernels"] = cnt["hbm_bytes"]
        # what the kernel is actually limited by: vector-instruction issue (one wave instruction per 4 cycles per SIMD), not HBM
        rf["limited_by"] = ("VALU issue, not HBM: the point-to-segment distance in the reference's mixed f32 / f64 is ~1 000 vector instructions per wave "
                            "and candidate batch — `valu_issue.frac` is the fraction that explains the time, `frac` (HBM) is reported because BASELINE's metric asks for it")
        rf["valu_issue"] = {"achieved": rf["valu_insts"] / (k_ms * 1e-3), "peak": 1024 * 2.4e9 / 4.0,
                            "unit": "VALU wave-instr/s (one per 4 cycles per SIMD)",
                            "frac": rf["valu_insts"] / (k_ms * 1e-3) / (1024 * 2.4e9 / 4.0)}
    else:
        out["synthetic_50k"]["roofline"]["traffic"] = None
    if cpu:
        out["cpu_baseline"] = lv_cpu(la3dm_amd, out)
    del m
    return out


def lv_cpu(la3dm_amd, leg, omp=False):
    """CPU leg of the BGK-LV sequence: 1 thread on the first 3 scans (the bounded sample), or — omp — the OpenMP build of
    the restatement (hits of the ray shortening and distinct blocks in parallel) on ALL 12 scans; the files are read
    before the clock starts"""
    from oracle import oracle as O
    params = dict(la3dm_amd.LV_YAML, resolution=0.05, block_depth=5)
    n = 12 if omp else 3
    scans = [la3dm_amd.load_pcd(os.path.join(ROOT, "tests", "golden", "data", "sim_unstructured", f"sim_unstructured_{i}.pcd"))
             for i in range(1, n + 1)]
    o = O.OracleLVMap(**params, omp=omp)
    t0 = time.perf_counter()
    for xyz, origin in scans:
        o.insert_pointcloud(xyz, origin, 0.05, 0.1, 8.0)
    tc = time.perf_counter() - t0
    return {"value": n / tc, "unit": "scans/s", "cores": O.lib(True).orc_num_threads() if omp else 1, "kind": "port",
            "sample": (f"all {n} scans" if omp else f"the first {n} of the 12 scans") + " into a fresh map of this repo's restatement ("
                      + ("OpenMP build" if omp else "1 thread") + "; clouds in memory before the clock starts)",
            "s_per_scan": tc / n, "gpu_scans_per_s": 12 / (leg["sequence_ms"] * 1e-3)}


def side_bench(args, torch, la3dm_amd, _lib):
    """--workload gp | lv | l: one leg on its own, wrapped in the contract keys (the default invocation carries all of
    them under "gp" / "lv" / "bgkl")"""
    torch.cuda.set_device(0)
    if args.workload == "l":
        leg = l_leg(args, torch, la3dm_amd, cpu=not args.no_cpu)
        value, unit, roof, ms = leg["voxel_updates_per_s"], "voxel-updates/s", leg["roofline"], leg["ms_per_step"]
    elif args.workload == "gp":
        leg = gp_leg(args, torch, la3dm_amd, _lib, depth=args.depth, cpu=not args.no_cpu)
        value, unit, roof, ms = leg["voxel_updates_per_s"], "voxel-updates/s", leg["roofline"], leg["ms_per_step"]
    else:
        leg = lv_leg(args, torch, la3dm_amd, _lib, cpu=not args.no_cpu)
        value, unit, roof, ms = 12.0 / (leg["sequence_ms"] * 1e-3), "scans/s", leg["synthetic_50k"]["roofline"], leg["sequence_ms"]
    print(json.dumps({"metric": "side bench (BASELINE configs[2] / configs[3] / row f4)", "value": value, "unit": unit, "n_gpus": 1,
                      "steps": leg.get("steps", 3), "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
                      "scaling": "none", "vs_baseline": None, "dtype": "f32",
                      "data": "sim_unstructured + synthetic" if args.workload == "lv" else "synthetic",
                      "config": {"workload": leg["workload"]}, "roofline": roof, "leg": leg}))


def l_leg(args, torch, la3dm_amd, cpu):
    """BGKLOctoMap (row f4) at the insert level: whole insert_pointcloud calls of the synthetic scan on the
    device-resident pool (front end with beam tags, rows, partition, predict + fuse incl. the split path, prune),
    the CPU restatement on all cores beside it."""
    params = dict(la3dm_amd.L_YAML, resolution=0.1, block_depth=3)
    rays = 200000
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    fr = 0.3
    m = la3dm_amd.BGKLOctoMap(**params, device=0)
    assert m.is_device_resident()
    # After a leg that released gigabytes of device memory ONE insert of the next map stalls for 10 - 80 ms somewhere in its first
    # dozen — no allocation, same work (tools/check/leg_order.py: it follows the release, whichever leg comes next).  Steady-state
    # loops show none: 1 500 inserts in a row, max 1.29 ms for this class, 0.82 ms for BGKOctoMap (tools/check/outliers.py,
    # profiles/r06/outliers.txt).  So the warm-up here is longer than the stall's window, every insert is timed on its own (it ends
    # with the host's read of the pass counters anyway) and the median is what is reported, with mean and max beside it.
    for _ in range(14):
        m.insert_pointcloud(xyz, origin, 0.1, fr, -1.0)
    steps = 10
    each = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.insert_pointcloud(xyz, origin, 0.1, fr, -1.0)
        torch.cuda.synchronize()
        each.append(time.perf_counter() - t0)
    dt = float(np.median(each))
    st = m.stats()
    U, rows = int(st["voxel_updates"]), int(st["train_reads"])
    b_alg = 32 * rows + 17 * U                     # a row (8 floats) per (tile, neighbour) pair + 17 B per leaf
    out = {"workload": f"BGKLOctoMap synthetic {rays}-ray scan re-inserted, 0.1 m, block_depth 3, bgkloctomap.yaml, "
                       f"free_resolution {fr}; a step = one insert_pointcloud (host cloud -> updated pool in HBM)",
           "ms_per_step": dt * 1e3, "ms_per_step_mean": float(np.mean(each)) * 1e3, "ms_per_step_max": float(np.max(each)) * 1e3,
           "timing": "median of the steps, each bracketed by a device synchronisation",
           "accumulate": ACC_SIDE[m.get_option("bgk_sum")],
           "voxel_updates_per_s": U / dt, "steps": steps,
           "voxel_updates_per_scan": U, "rows_read_per_scan": rows, "pair_evals_per_scan": int(st["pair_evals"]),
           "test_blocks": int(st["n_test_blocks"]),
           "roofline": {"bound": "hbm", "achieved": b_alg / dt / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": b_alg / dt / 1e9 / 8000.0, "traffic": None, "kernel": "insert_pointcloud (all kernels)",
                        "kernel_ms": dt * 1e3, "algorithmic_bytes_per_launch": b_alg}}
    cnt = profiled_counters("l", path="side_counters.json", sources=("bgkl_kernels.h",))
    if cnt:   # HBM bytes of one insert, all kernels (tools/prof/side_pmc.sh: FETCH_SIZE x 2 + WRITE_SIZE, separate --pmc passes)
        out["roofline"]["traffic"] = cnt["hbm_bytes"]
        out["roofline"]["traffic_source"] = cnt.get("source")
        # the part of it the algorithmic bytes describe: the inference kernels (rows x tiles -> sums -> update); the rest is
        # the insert's front end, partition, leaf lists, commit and prune
        out["roofline"]["traffic_inference_kernels"] = sum((2 * e.get("FETCH_SIZE", 0.0) + e.get("WRITE_SIZE", 0.0)) * 1024
                                                            for k, e in cnt["kernels"].items() if "bgkl_" in k and "rows_prepare" not in k)
        out["roofline"]["valu_insts"] = cnt.get("valu_insts")
        if cnt.get("valu_insts"):
            out["roofline"]["valu_issue"] = {"achieved": cnt["valu_insts"] / dt, "peak": 1024 * 2.4e9 / 4.0,
                                             "unit": "VALU wave-instr/s (one per 4 cycles per SIMD), all kernels of the insert",
                                             "frac": cnt["valu_insts"] / dt / (1024 * 2.4e9 / 4.0)}
    if cpu:
        out["cpu_baseline"] = l_cpu(la3dm_amd)
    del m
    return out


def l_cpu(la3dm_amd):
    from oracle import oracle as O
    params = dict(la3dm_amd.L_YAML, resolution=0.1, block_depth=3)
    xyz, origin = la3dm_amd.synthetic_scan(200000)
    o = O.OracleLMap(**params, omp=True)
    o.insert_pointcloud(xyz, origin, 0.1, 0.3, -1.0)
    t0 = time.perf_counter()
    o.insert_pointcloud(xyz, origin, 0.1, 0.3, -1.0)
    tc = time.perf_counter() - t0
    return {"value": float(o.stats()["voxel_updates"]) / tc, "unit": "voxel-updates/s",
            "cores": O.lib(True).orc_num_threads(), "kind": "port",
            "sample": "the same scan re-inserted once into the OpenMP build of this repo's restatement",
            "insert_pointcloud_s": tc}


SEQ_POSES = [None, (1.5, 0.5, 1.0), (-1.5, 1.0, 1.2), (0.5, -2.0, 0.9), (2.5, 2.0, 1.1)]   # sensor poses of the e2e sequence


def e2e_sequence(la3dm_amd, rays):
    return [la3dm_amd.synthetic_scan(rays, origin=p) for p in SEQ_POSES]


def end_to_end(la3dm_amd, params, args):
    """Whole BGKOctoMap::insert_pointcloud calls in device-resident mode (front end, partition, predict + fuse,
    write-back, prune on the GPU; the cloud is uploaded from host memory inside the timed region), like for like with
    the CPU leg (cpu_baseline_omp.sequence): scan 0 goes into a FRESH map (timed on its own: block creation and the first
    growth of the device arenas are in it), then four more scans of the same room from other sensor poses follow into
    the same map (distinct scans, no re-insertion)."""
    import torch
    scans = e2e_sequence(la3dm_amd, args.rays)
    la3dm_amd.BGKOctoMap(**params, device=0).insert_pointcloud(*scans[0], args.resolution, 0.5, -1.0)   # library warm-up
    torch.cuda.synchronize()
    # the whole sequence kReps times, each into a fresh map; per position the MEDIAN over the repeats (a single sample of the
    # first insert was at the mercy of one host hiccup: 71 ms once, 1.3 ms in 40 of 40 repeats of the same call)
    kReps = 3
    d_clouds = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0") for x, _ in scans]
    all_t, all_td = [], []
    for rep in range(kReps):
        m = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(True)
        torch.cuda.synchronize()
        times, updates = [], []
        for xyz, origin in scans:
            t0 = time.perf_counter()
            m.insert_pointcloud(xyz, origin, args.resolution, 0.5, -1.0)
            times.append(time.perf_counter() - t0)
            updates.append(int(m.stats()["voxel_updates"]))
        st = m.stats()
        all_t.append(times)
        # the same sequence with the clouds already resident in HBM (insert_pointcloud_device), another fresh map
        m2 = la3dm_amd.BGKOctoMap(**params, device=0).set_device_resident(True)
        torch.cuda.synchronize()
        times_dev = []
        for d, (_, origin) in zip(d_clouds, scans):
            t0 = time.perf_counter()
            m2.insert_pointcloud_device(d.data_ptr(), d.shape[0], origin, args.resolution, 0.5, -1.0)
            times_dev.append(time.perf_counter() - t0)
        all_td.append(times_dev)
        del m, m2
    times = [float(x) for x in np.median(np.array(all_t), axis=0)]
    times_dev = [float(x) for x in np.median(np.array(all_td), axis=0)]
    seq, seq_dev = float(np.mean(times[1:])), float(np.mean(times_dev[1:]))
    return {"what": "BGKOctoMap.insert_pointcloud, device-resident map, host cloud -> updated pool in HBM (PCIe upload of the "
                    "cloud included): scan 0 into a fresh map, then 4 distinct scans (other sensor poses) into the same map; "
                    "*_device_cloud: the clouds already in HBM",
            "first_insert_fresh_map_ms": times[0] * 1e3, "ms_per_insert": seq * 1e3,
            "voxel_updates_per_s": float(np.mean(updates[1:])) / seq,
            "first_insert_fresh_map_ms_device_cloud": times_dev[0] * 1e3, "ms_per_insert_device_cloud": seq_dev * 1e3,
            "voxel_updates_per_s_device_cloud": float(np.mean(updates[1:])) / seq_dev,
            "ms_each": [t * 1e3 for t in times], "voxel_updates_each": updates, "calls": len(scans),
            "repeats": kReps, "timing": "per position of the sequence, the median over the repeats (each into a fresh map)",
            "stages_s_last_call": {"frontend": st["t_frontend"], "partition": st["t_partition"],
                                   "pack_kernel_commit_prune": st["t_pack"]}}


def packed_kernel_leg(la3dm_amd, _lib, torch, dev, rays, res, depth, workload, steps=10, options=None):
    """la3dm_bgk_scan_device on another packed scan resident in HBM (same protocol as the headline step): kernel time by HIP
    events, algorithmic bytes, pair evaluations; `options` = la3dm_set_option pairs applied for this leg only"""
    params = dict(la3dm_amd.BGK_YAML, resolution=res, block_depth=depth)
    xyz, origin = la3dm_amd.synthetic_scan(rays)
    m = la3dm_amd.BGKOctoMap(**params, device=0)
    assert m.prepare(xyz, origin, res, 0.5, -1.0)
    st, pk = m.stats(), m.packed()
    U = int(st["voxel_updates"])
    b_alg = 16 * int(st["train_reads"]) + 17 * U
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
            (pk.train_xyzy, pk.train_off.view(np.int32), pk.nbr, pk.blk_center, pk.leaf_off.view(np.int32),
             pk.leaf_key.view(np.int32), pk.alpha, pk.beta)]
    state = torch.zeros(pk.n_leaf, dtype=torch.uint8, device=dev)
    scan = _lib.BgkScan()
    (scan.train_xyzy, scan.train_off, scan.nbr, scan.blk_center, scan.leaf_off, scan.leaf_key, scan.alpha,
     scan.beta) = [t.data_ptr() for t in keep]
    scan.state = state.data_ptr()
    scan.n_train_pts, scan.n_train_blk, scan.n_test_blk, scan.n_leaf, scan.flags = pk.n_train_pts, pk.n_train_blk, pk.n_test_blk, pk.n_leaf, pk.flags
    H = _lib.hip()
    stream = torch.cuda.current_stream().cuda_stream
    for k, v in (options or {}).items():
        m.set_option(k, v)
    for _ in range(2):
        assert H.la3dm_bgk_scan_device(m.ctx(), C.byref(scan), stream, None) == 0
    m.set_option("time_kernel", 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        assert H.la3dm_bgk_scan_device(m.ctx(), C.byref(scan), stream, None) == 0
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    kt = np.zeros(steps + 8, np.float32)
    nk = C.c_uint32()
    H.la3dm_kernel_times(m.ctx(), kt.ctypes.data, kt.size, C.byref(nk))
    m.set_option("time_kernel", 0)
    k_ms = float(kt[:nk.value].mean())
    ach = b_alg / (k_ms * 1e-3) / 1e9
    sum_mode = m.get_option("bgk_sum")
    out = {"workload": workload, "kernel": kernel_name(m, sum_mode, scan.flags, pk),
           "voxel_updates_per_scan": U, "test_blocks": int(pk.n_test_blk), "pair_evals_per_scan": int(st["pair_evals"]),
           "algorithmic_bytes_per_launch": b_alg, "kernel_ms": k_ms, "ms_per_step": dt * 1e3,
           "voxel_updates_per_s": U / dt, "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": ach / 8000.0,
           "pair_evals_per_s": int(st["pair_evals"]) / (k_ms * 1e-3), "steps": steps}
    counters = profiled_counters(f"rays{rays}_d{depth}_r{res}_sum{sum_mode}")
    if counters and not options:
        n_valu, n_salu, n_lds = (counters.get(k, 0) for k in ("valu_insts_per_launch", "salu_insts_per_launch", "lds_insts_per_launch"))
        simds, clk = 1024, 2.4e9
        out["traffic"] = counters.get("hbm_bytes_per_launch")
        out["issue"] = {"valu_insts_per_launch": n_valu, "salu_insts_per_launch": n_salu, "lds_insts_per_launch": n_lds,
                        "valu_per_tile": n_valu / max(1.0, counters.get("waves_per_launch") or 1.0),
                        "frac": (n_valu + n_salu + n_lds) / (k_ms * 1e-3) / (simds * clk / 2.2),
                        "valu_frac_4cycle": n_valu / (k_ms * 1e-3) / (simds * clk / 4.1), "source": counters.get("source")}
    return out


def out_of_cache_leg(la3dm_amd, _lib, torch, dev):
    """The same kernel on configs[4]'s scan (1M rays, 0.05 m, depth 3) on this one GPU: B_alg ~ 0.58 GB per launch and a
    working set beyond the 256 MiB Infinity Cache, so achieved GB/s here is a genuine HBM-side figure (at configs[1] the
    ~45 MB working set stays cache resident across the in-place steps)."""
    return packed_kernel_leg(la3dm_amd, _lib, torch, dev, 1000000, 0.05, 3,
                             "BGKOctoMap synthetic 1000000-ray scan, 0.05 m, block_depth 3 (configs[4] on one GPU)")


def depth4_leg(la3dm_amd, _lib, torch, dev):
    """configs[1]'s scan at block_depth 4 — the reference constructor's default (src/bgkoctomap/bgkoctomap.cpp:20-29; SURVEY 8d
    and BASELINE.md ask for both depths): 0.8 m blocks of 512 leaves = eight 64-leaf tiles per test block, each with the block's
    7-neighbourhood as candidates; ~8x the pair evaluations of depth 3 for ~1.2x the algorithmic bytes, so the HBM fraction is
    far lower by construction — the issue fraction says how busy the SIMDs are"""
    return packed_kernel_leg(la3dm_amd, _lib, torch, dev, 200000, 0.1, 4,
                             "BGKOctoMap synthetic 200000-ray scan, 0.1 m, block_depth 4 (configs[1] at the reference constructor's default depth)")


def kernel_variants_leg(la3dm_amd, _lib, torch, dev):
    """what a cheaper kernel FUNCTION would buy.  The same launch (configs[1]; configs[4] out of cache) with the
    evaluation swapped: the default (correctly rounded sqrt / sin / cos: bit-identical k), fast_trig 3 (Eigen 3.3.7 psin / pcos,
    fp32 only, no f64 chain: the likely reference build's values), fast_trig 1 (fp32 polynomial, <= 1.5 ulp), and `ablate` 1 —
    NO evaluation at all (results invalid: the floor any evaluation, however cheap, sits on)."""
    rows = {}
    for name, opts in (("default", None), ("fast_trig_3", {"fast_trig": 3}), ("fast_trig_1", {"fast_trig": 1}),
                       ("no_evaluation(ablate 1, invalid results)", {"ablate": 1}),
                       ("no_tests_no_evaluation(ablate 2, invalid results)", {"ablate": 2})):
        a = packed_kernel_leg(la3dm_amd, _lib, torch, dev, 200000, 0.1, 3, "configs[1]", steps=20, options=opts)
        b = packed_kernel_leg(la3dm_amd, _lib, torch, dev, 1000000, 0.05, 3, "configs[4]", steps=6, options=opts)
        rows[name] = {"configs1_kernel_us": a["kernel_ms"] * 1e3, "configs1_frac": a["frac"], "configs1_kernel": a["kernel"],
                      "out_of_cache_kernel_us": b["kernel_ms"] * 1e3, "out_of_cache_frac": b["frac"]}
    return rows


def cpu_baseline(params, xyz, origin, args, U, omp=False):
    """The CPU oracle (strict-fp32 restatement of the reference's insert_pointcloud) on the same
    scan, on this box's host cores.  Bounded: for the default 200k-ray scan one full
    insert_pointcloud takes ~10-20 s on one core; larger workloads are subsampled by rays.
    The all-core leg also runs end_to_end's five-scan sequence into one fresh map (`sequence`)."""
    from oracle import oracle as O
    rays = xyz.shape[0]
    sample = xyz
    desc = f"full {rays}-ray scan, 1 insert_pointcloud into a fresh map"
    if rays > 250000 and not omp:
        sample = xyz[:: int(np.ceil(rays / 250000))]
        desc = f"every {int(np.ceil(rays / 250000))}th ray of the scan ({sample.shape[0]} rays), 1 insert_pointcloud into a fresh map"
    # single core: one insert (~6 s at the default workload); all cores: one warm-up + the median of five fresh maps
    runs = []
    for rep in range(6 if omp else 1):
        o = O.OracleMap(**params, omp=omp)
        t0 = time.perf_counter()
        o.insert_pointcloud(sample, origin, args.resolution, 0.5, -1.0)
        runs.append((time.perf_counter() - t0, o.stats()))
    if omp:
        runs = sorted(runs[1:], key=lambda r: r[1]["t_predict"])
        desc += ", median of 5 after 1 warm-up"
    t, s = runs[len(runs) // 2]
    cores = O.lib(omp).orc_num_threads() if omp else 1
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except Exception:
        pass
    out = {"value": s["voxel_updates"] / s["t_predict"], "unit": "voxel-updates/s", "cores": cores, "kind": "port",
           "sample": desc + "; value = leaves of test blocks / predict+fuse stage time",
           "stage_s": {"frontend": s["t_frontend"], "partition": s["t_partition"], "predict_fuse": s["t_predict"],
                       "prune": s["t_prune"], "insert_pointcloud": t},
           "voxel_updates": s["voxel_updates"], "host_cpus": os.cpu_count(), "host_cpu_model": cpu}
    if omp and rays <= 250000 and not args.no_e2e:
        import la3dm_amd
        o = O.OracleMap(**params, omp=True)
        ts = []
        for sx, so in e2e_sequence(la3dm_amd, rays):
            t0 = time.perf_counter()
            o.insert_pointcloud(sx, so, args.resolution, 0.5, -1.0)
            ts.append(time.perf_counter() - t0)
        out["sequence"] = {"what": "end_to_end's five-scan sequence into one fresh oracle map, same host cores",
                           "first_insert_fresh_map_s": ts[0], "s_per_insert": float(np.mean(ts[1:])), "s_each": ts}
    return out


if __name__ == "__main__":
    main()
