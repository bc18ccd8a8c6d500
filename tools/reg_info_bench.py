"""Measurement of registration information (fbr_reg_info_poses, fbr_batch_info) on the C2 workload:
  * one info pass on a single 64x1800 scan: the call and its kernels (fbr_set_profiling), beside the
    gn_knn + gn_residual time of one Gauss-Newton iteration of a registration of the same scan in the
    same run (one pass does an iteration's work without the fit cache and the warm start);
  * fbr_batch_info of a B-job batch (its host part: the clouds down, a sort per job, the clouds up)
    beside one batch launch of the same jobs.
usage: reg_info_bench.py [reps] [--batch B] [--batch-reps N] [--distinct K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from feature_base_pointcloud_registration_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=20)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--batch-reps", type=int, default=5)
ap.add_argument("--distinct", type=int, default=16)  # distinct scans of the batch (the rest repeat them)
args = ap.parse_args()
reps = args.reps
INFO = ("reg_info_items", "reg_info_jobs")
GN = ("gn_knn", "gn_residual", "gn_loop")
H, W = synth.CONFIGS["C2"][:2]
res = {"reps": reps, "batch": args.batch, "batch_reps": args.batch_reps}


def kernel_ms(ctx, names, call, n):
    """Mean kernel time per call of each name over n calls, and the launches per call."""
    ctx.set_profiling(True, names)
    before = {k: ctx.kernel_time(k) for k in names}
    out = [call() for _ in range(n)]
    after = {k: ctx.kernel_time(k) for k in names}
    ctx.set_profiling(False)
    return ({k: round((after[k][0] - before[k][0]) / n, 5) for k in names},
            {k: (after[k][1] - before[k][1]) / n for k in names}, out)


# ---- one scan ----
P = synth.config_params("C2")
gt, guess = synth.job(9000)
scan = synth.scan(gt, H, W, seed=9000)
with api.Context(P) as ctx:
    ctx.set_map(*synth.config_map("C2"))
    f = ctx.features(scan)
    corner = ctx.voxel_grid(f["corner"], P.mapping_corner_leaf_size)
    surf = ctx.voxel_grid(f["surf"], P.mapping_surf_leaf_size)
    pose, st = ctx.register(f["corner"], f["surf"], guess)
    rec = ctx.reg_info(corner, surf, pose[None])  # warm-up: allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.reg_info(corner, surf, pose[None])
    call_ms = (time.perf_counter() - t0) / reps * 1e3
    kern, _, _ = kernel_ms(ctx, INFO, lambda: ctx.reg_info(corner, surf, pose[None]), reps)
    gn, launches, sts = kernel_ms(ctx, GN, lambda: ctx.register(f["corner"], f["surf"], guess)[1], reps)
    iters = float(np.mean([s["iterations"] for s in sts]))
    gn_iter = sum(gn.values()) / iters
    res["single"] = {"queries": [len(corner), len(surf)], "n_rows": rec[0]["n_rows"].tolist(), "rank": int(rec[0]["rank"]),
                     "call_ms": round(call_ms, 4), "kernel_ms": kern, "register_iterations": iters,
                     "gn_kernel_ms_per_register": gn, "gn_knn_residual_ms_per_iteration": round(gn_iter, 5),
                     "info_kernels_over_one_iteration": round(sum(kern.values()) / gn_iter, 3)}

# ---- a batch ----
B = args.batch
PB = synth.config_params("C2", max_batch=B)
jobs = [synth.job(9100 + k) for k in range(args.distinct)]
scans = [synth.scan(j[0], H, W, seed=9100 + k) for k, j in enumerate(jobs)]
bs = [scans[k % args.distinct] for k in range(B)]
bg = np.asarray([jobs[k % args.distinct][1] for k in range(B)], np.float32)
with api.Context(PB) as ctx:
    ctx.set_map(*synth.config_map("C2"))
    ctx.batch_stage(bs, bg)
    ctx.batch_launch()
    ctx.batch_wait()  # warm-up
    t0 = time.perf_counter()
    for _ in range(args.batch_reps):
        ctx.batch_launch()
        ctx.batch_wait()
    launch_ms = (time.perf_counter() - t0) / args.batch_reps * 1e3
    info = ctx.batch_info()  # warm-up: allocations
    t0 = time.perf_counter()
    for _ in range(args.batch_reps):
        ctx.batch_info()
    info_ms = (time.perf_counter() - t0) / args.batch_reps * 1e3
    kern, _, _ = kernel_ms(ctx, INFO, ctx.batch_info, args.batch_reps)
    res["batch"] = {"jobs": B, "launch_wait_ms": round(launch_ms, 3), "batch_info_ms": round(info_ms, 3), "kernel_ms": kern,
                    "host_ms": round(info_ms - sum(kern.values()), 3), "batch_info_over_launch": round(info_ms / launch_ms, 3),
                    "info_kernels_over_launch": round(sum(kern.values()) / launch_ms, 3),
                    "mean_queries": [float(info["n_query"][:, 0].mean()), float(info["n_query"][:, 1].mean())],
                    "flagged": int((info["flags"] != 0).sum())}
print(json.dumps(res))
