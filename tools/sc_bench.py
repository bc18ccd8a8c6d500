"""Measurement of the place-recognition path (fbr_sc_update, fbr_sc_query): the describe time of
1,000 C2-sized keyframes, the query time against 1,000 and 10,000 stored descriptors, and the search
kernel's achieved bytes/s against its bytes model (n_ring n_sector 4 + n_sector 8 bytes per
candidate).  The keyframe clouds are a few real C2 feature clouds (64 x 1800 scans, mapping-leaf
VoxelGrids) turned about z by random angles, so every keyframe has its own dense descriptor.
usage: sc_bench.py [n_describe] [n_large] [reps] [n_base_scans]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "oracle"))
from feature_base_pointcloud_registration_amd import api, synth  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, sc_params  # noqa: E402
import pyoracle as O  # noqa: E402

n_desc = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
n_large = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
n_base = int(sys.argv[4]) if len(sys.argv) > 4 else 6
P = synth.config_params("C2")
H, W = synth.CONFIGS["C2"][:2]
rng = np.random.default_rng(0)
base = []
for k in range(n_base):
    gt, _ = synth.job(7000 + k)
    f = O.Stream(P).features(synth.scan(gt, H, W, seed=7000 + k))
    base.append((O.voxel_grid(f["corner"], P.mapping_corner_leaf_size), O.voxel_grid(f["surf"], P.mapping_surf_leaf_size)))


def turned(cloud, a, keep=None):
    out = cloud.copy() if keep is None else cloud[rng.choice(len(cloud), min(keep, len(cloud)), replace=False)].copy()
    x, y = out["x"].copy(), out["y"].copy()
    out["x"], out["y"] = np.cos(a) * x - np.sin(a) * y, np.sin(a) * x + np.cos(a) * y
    return out


def add(ctx, n, keep=None):
    pts = 0
    for _ in range(n):
        c, s = base[int(rng.integers(n_base))]
        a = rng.uniform(-np.pi, np.pi)
        c, s = turned(c, a, None if keep is None else keep // 8), turned(s, a, keep)
        ctx.keyframes_add(np.zeros(1, KEYPOSE)[0], c, s)
        pts += len(c) + len(s)
    return pts


def kernel_split(ctx, names, fn, n):
    before = {k: ctx.kernel_time(k) for k in names}
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    wall = (time.perf_counter() - t0) / n
    out = {}
    for k in names:
        ms, cnt = ctx.kernel_time(k)
        out[k] = {"ms_per_call": round((ms - before[k][0]) / n, 5), "launches_per_call": (cnt - before[k][1]) / n}
    return wall, out


names = ("sc_describe", "sc_norms", "sc_search")
sp = sc_params()
cell_bytes = sp.n_ring * sp.n_sector * 4 + sp.n_sector * 8
res = {"n_ring": sp.n_ring, "n_sector": sp.n_sector, "bytes_per_candidate": cell_bytes}
with api.Context(P) as ctx:
    pts = add(ctx, n_desc)
    res["describe_keyframes"] = n_desc
    res["describe_points"] = pts
    ctx.sc_update(sp)  # warm-up: allocations
    # another lidar_height discards the store: every update below describes all keyframes again
    heights = [2.0 + 0.001 * (i + 1) for i in range(reps)]
    t0 = time.perf_counter()
    for h in heights:
        assert ctx.sc_update(sc_params(lidar_height=h)) == n_desc
    res["describe_call_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 4)
    ctx.set_profiling(True, names)
    _, split = kernel_split(ctx, names, lambda i: ctx.sc_update(sc_params(lidar_height=3.0 + 0.001 * i)), reps)
    ctx.set_profiling(False)
    res["describe_kernels"] = split
    res["describe_read_GBps"] = round(pts * 16 / (split["sc_describe"]["ms_per_call"] * 1e-3) / 1e9, 2)
    qc, qs = turned(base[0][0], 0.3), turned(base[0][1], 0.3)
    res["query_points"] = len(qc) + len(qs)
    for n in (n_desc, n_large):
        have = ctx.keyframes_count()
        if n > have:
            add(ctx, n - have, keep=2000)  # small clouds: only the number of descriptors matters to the search
        ctx.sc_update(sp)
        ctx.sc_query(qc, qs, 16, sp)  # warm-up
        t0 = time.perf_counter()
        for _ in range(reps):
            m = ctx.sc_query(qc, qs, 16, sp)
        wall = (time.perf_counter() - t0) / reps
        ctx.set_profiling(True, names)
        _, split = kernel_split(ctx, names, lambda i: ctx.sc_query(qc, qs, 16, sp), reps)
        ctx.set_profiling(False)
        ms = split["sc_search"]["ms_per_call"]
        res["query_N%d" % n] = {"call_ms": round(wall * 1e3, 4), "kernels": split, "best": [m[0]["keyframe"], m[0]["shift"],
                                                                                          round(m[0]["distance"], 4)],
                                "search_model_bytes": n * cell_bytes,
                                "search_GBps": round(n * cell_bytes / (ms * 1e-3) / 1e9, 2) if ms > 0 else None}
print(json.dumps(res))
