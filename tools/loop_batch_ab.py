"""A/B of loop closure for many keyframe pairs: the loop of single calls against one
fbr_perform_loop_closures call.

The store is the out-and-back run of tests/test_loop_closure.py driven `laps` times (16x1800 synth
scans, 20 keyframes a lap, each lap 0.1 m beside the previous one, a few centimetres of stored-pose
drift per keyframe), about 200 keyframes; the pairs are fbr_loop_candidates' with the default loop
parameters but search_num (default 3).  Timed, three interleaved repetitions after a warm-up:
  single   fbr_perform_loop_closure at every keyframe while the store grows (the store then holds
           keyframes 0..i: the single call for pair i); only the calls are timed, not the adds
  chunk1   fbr_perform_loop_closures with chunk_pairs = 1
  batch    fbr_perform_loop_closures with chunk_pairs = 0
and, in a separate profiled pass (fbr_set_profiling), the device time of the ICP kernels (icp_nn,
icp_nn_far, icp_solve: the iterations and the fitness pass) of each, so that the rest of a call
(transforms, VoxelGrids, grid builds, copies, host) can be told from the iterations.
The three must return the same bytes; the tool checks it.

usage: loop_batch_ab.py [--laps N] [--search-num K] [--cache FILE.npz] [--out FILE]
  --cache: keep the keyframe clouds (the CPU oracle's features of the synth scans) in FILE.npz
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "oracle"))
from feature_base_pointcloud_registration_amd import api, synth  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, default_params, loop_params  # noqa: E402

NAMES = ("icp_nn", "icp_nn_far", "icp_solve")
H, W = 16, 1800


def gt_pose(k):
    lap, q = divmod(k, 20)
    s = q if q < 10 else 19 - q
    return np.array([0.0, 0.0, 0.02 * s, 1.5 * s, 0.3 * np.sin(0.5 * s) + (0.4 if q >= 10 else 0.0) + 0.1 * lap, 0.0])


def build_store(P, n, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if int(z["n"]) == n:
            return z["poses"], [z["c%d" % k] for k in range(n)], [z["s%d" % k] for k in range(n)]
    import pyoracle as O
    rng = np.random.default_rng(7)
    poses = np.zeros(n, KEYPOSE)
    corners, surfs = [], []
    for k in range(n):
        gt = gt_pose(k)
        f = O.Stream(P).features(synth.scan(gt, H, W, seed=100 + k))
        corners.append(O.voxel_grid(f["corner"], P.mapping_corner_leaf_size))
        surfs.append(O.voxel_grid(f["surf"], P.mapping_surf_leaf_size))
        d = rng.normal(0.0, 1.0, 4) * (0.01, 0.08, 0.08, 0.03)  # stored-pose drift: yaw, x, y, z
        poses[k] = (gt[3] + d[1], gt[4] + d[2], gt[5] + d[3], k, gt[0], gt[1], gt[2] + d[0], 0.0, 2.0 * k)
    if cache:
        np.savez(cache, n=n, poses=poses, **{"c%d" % k: corners[k] for k in range(n)},
                 **{"s%d" % k: surfs[k] for k in range(n)})
    return poses, corners, surfs


def raw(r):
    return ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def icp_ms(ctx):
    return sum(ctx.kernel_time(n)[0] for n in NAMES), sum(ctx.kernel_time(n)[1] for n in NAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=10)
    ap.add_argument("--search-num", type=int, default=3)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = 20 * a.laps
    P = default_params(H, W)
    poses, corners, surfs = build_store(P, n, a.cache)
    lp = loop_params(search_num=a.search_num)

    with api.Context(P) as full, api.Context(P) as grow:
        for k in range(n):
            full.keyframes_add(poses[k], corners[k], surfs[k])
        pairs = full.loop_candidates(lp)
        latest = {i for i, _ in pairs}

        def single():
            """The single call at every keyframe with a candidate while the store grows; returns
            (seconds in the calls, results)."""
            grow.keyframes_reset()
            t, out = 0.0, []
            for k in range(n):
                grow.keyframes_add(poses[k], corners[k], surfs[k])
                if k in latest:
                    t0 = time.perf_counter()
                    out.append(grow.perform_loop_closure(float(poses["time"][k]), lp, raw=True))
                    t += time.perf_counter() - t0
            return t, out

        def batch(chunk):
            t0 = time.perf_counter()
            out = full.perform_loop_closures(pairs, lp, chunk=chunk, raw=True)
            return time.perf_counter() - t0, out

        # warm-up (allocations), and the three must agree
        _, rs = single()
        _, r1 = batch(1)
        _, r0 = batch(0)
        assert [(r.latest_id, r.closest_id) for r in rs] == pairs
        same = [raw(x) == raw(y) == raw(z) for x, y, z in zip(rs, r1, r0)]
        times = {"single": [], "chunk1": [], "batch": []}
        for _ in range(3):
            times["single"].append(single()[0])
            times["chunk1"].append(batch(1)[0])
            times["batch"].append(batch(0)[0])
        # the profiled pass: device time of the ICP kernels
        prof = {}
        for name, ctx, run in (("single", grow, single), ("chunk1", full, lambda: batch(1)), ("batch", full, lambda: batch(0))):
            ctx.set_profiling(True, NAMES)
            b_ms, b_n = icp_ms(ctx)
            t = run()[0]
            ms, cnt = icp_ms(ctx)
            ctx.set_profiling(False)
            prof[name] = {"wall_ms": round(t * 1e3, 3), "icp_kernel_ms": round(ms - b_ms, 3), "icp_launches": cnt - b_n}
    its = [r.icp.iterations for r in r0]
    res = {"keyframes": n, "pairs": len(pairs), "search_num": a.search_num, "bytes_equal": all(same),
           "closed": sum(r.status == 0 for r in r0), "iterations_sum": int(sum(its)), "iterations_max": int(max(its)),
           "n_source": [int(min(r.n_source for r in r0)), int(max(r.n_source for r in r0))],
           "n_target": [int(min(r.n_target for r in r0)), int(max(r.n_target for r in r0))],
           "wall_ms": {k: [round(v * 1e3, 3) for v in t] for k, t in times.items()}, "profiled": prof}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
