"""Measurement of pose scoring (fbr_score_poses): poses/s and queries/s on the C1 and C2 maps for
n_poses in {1, 64, 4096}, the kernel times from fbr_set_profiling, the search kernel's register count
(hipcc -S + tools/kernel_resources.py) and, for scale, the time of `top` sequential register() calls
on the same scan: what a caller without the score spends per hypothesis.  The scan's features are
extracted and down-sampled on the device; the poses are drawn within +-3 m / +-0.8 rad of the truth.
usage: score_bench.py [reps] [top] [--resources-only] [--chunk N]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from feature_base_pointcloud_registration_amd import api, build, synth  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import score_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("top", nargs="?", type=int, default=3)
ap.add_argument("--chunk", type=int, default=0)
ap.add_argument("--resources-only", action="store_true")
args = ap.parse_args()
reps, top, chunk = args.reps, args.top, args.chunk


def resources():
    """VGPR / SGPR / LDS of the k_score.hip kernels, from the assembly hipcc writes for them."""
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "k_score.s")
        subprocess.check_call([build.hipcc(), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", f"--offload-arch={build.ARCH}",
                               "-I", build.CSRC, "-I", os.path.join(R, "include"), "--cuda-device-only", "-S",
                               os.path.join(build.CSRC, "k_score.hip"), "-o", asm], stderr=subprocess.DEVNULL)
        out = subprocess.check_output([sys.executable, os.path.join(R, "tools", "kernel_resources.py"), asm], text=True)
    return [" ".join(ln.split()) for ln in out.splitlines()]


if args.resources_only:
    print(json.dumps({"kernel_resources": resources()}))
    sys.exit(0)

names = ("score_nn", "score_sum")
res = {"reps": reps, "top": top, "pose_chunk": chunk or 1024}
rng = np.random.default_rng(0)
for cfg in ("C1", "C2"):
    P = synth.config_params(cfg)
    H, W = synth.CONFIGS[cfg][:2]
    gt, guess = synth.job(9000)
    scan = synth.scan(gt, H, W, seed=9000)
    out = {}
    with api.Context(P) as ctx:
        ctx.set_map(*synth.config_map(cfg))
        info = ctx.map_grid_info()
        out["map_points"] = [info["n_corner"], info["n_surf"]]
        out["grid"] = {"sparse": info["sparse"], "dims": info["dims"]}
        f = ctx.features(scan)
        corner = ctx.voxel_grid(f["corner"], P.mapping_corner_leaf_size)
        surf = ctx.voxel_grid(f["surf"], P.mapping_surf_leaf_size)
        npts = len(corner) + len(surf)
        out["scan_points"] = [len(corner), len(surf)]
        sp = score_params(pose_chunk=chunk)
        for n in (1, 64, 4096):
            poses = np.tile(np.asarray(gt, np.float32), (n, 1))
            poses[:, 3:5] += rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32)
            poses[:, 2] += rng.uniform(-0.8, 0.8, n).astype(np.float32)
            sc = ctx.score_poses(corner, surf, poses, sp)  # warm-up: allocations
            r = max(2, reps if n < 4096 else reps // 3)
            t0 = time.perf_counter()
            for _ in range(r):
                ctx.score_poses(corner, surf, poses, sp)
            wall = (time.perf_counter() - t0) / r
            ctx.set_profiling(True, names)
            before = {k: ctx.kernel_time(k) for k in names}
            for _ in range(r):
                ctx.score_poses(corner, surf, poses, sp)
            kern = {k: round((ctx.kernel_time(k)[0] - before[k][0]) / r, 5) for k in names}
            ctx.set_profiling(False)
            nn_s = kern["score_nn"] * 1e-3
            out["n%d" % n] = {"call_ms": round(wall * 1e3, 4), "poses_per_s": round(n / wall, 1),
                              "queries_per_s": round(n * npts / wall, 1), "kernel_ms": kern,
                              "kernel_queries_per_s": round(n * npts / nn_s, 1) if nn_s > 0 else None,
                              "inlier_share": round(float(sc["n_in"].sum() / max(sc["n"].sum(), 1)), 4),
                              "fitness_min_max": [round(float(sc["fitness"].min()), 5), round(float(sc["fitness"].max()), 5)]}
        # the scale: `top` registrations one after another, from the guess (a seed registration can use)
        ctx.register(f["corner"], f["surf"], guess)
        t0 = time.perf_counter()
        for _ in range(reps):
            for _ in range(top):
                pose, st = ctx.register(f["corner"], f["surf"], guess)
        out["register_top_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 4)
        out["register_iterations"] = st["iterations"]
        out["fitness_at_truth"] = round(float(ctx.score_poses(corner, surf, np.asarray(gt, np.float32)[None], sp)[0]["fitness"]), 5)
        out["fitness_registered"] = round(float(ctx.score_poses(corner, surf, pose[None], sp)[0]["fitness"]), 5)
    res[cfg] = out
try:
    res["kernel_resources"] = resources()
except (OSError, subprocess.CalledProcessError, RuntimeError) as e:  # no compiler here: the counts are static
    res["kernel_resources"] = "unavailable: %s" % type(e).__name__
print(json.dumps(res))
