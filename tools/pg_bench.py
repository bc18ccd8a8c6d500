"""Measurement of the pose-graph optimiser (fbr_pg_optimize): synthetic keyframe chains of N nodes
with K loop factors, the time per optimise, the Levenberg-Marquardt steps, the PCG iterations and the
per-launcher kernel times (fbr_set_profiling), and the same graphs through the CPU probe's host
solve (tests/native/pg_probe.cpp, one thread) for scale.  There is no pass bar: the table
(profiles/pose_graph.md) is the record.  One JSON line per case.
usage: pg_bench.py [reps] [N,N,...] [K,K,...] [K of the extra many-loops case at the largest N]"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
from feature_base_pointcloud_registration_amd import api  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params  # noqa: E402
import pg_fixtures as F  # noqa: E402
import pg_model as PM  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1000, 10000]
loops = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1, 10]
many = int(sys.argv[4]) if len(sys.argv) > 4 else 200
NAMES = ("pg_linearize", "pg_assemble", "pg_factor", "pg_pcg", "pg_retract")


def graph(n, k):
    """A circle of ~1 m steps (2e-3 rad / 0.02 m odometry noise, yaw bias 1e-5 rad per step) with k
    loop factors spread over it: (n - 1, 0) first, the others pair a late node with an early one."""
    step = max(1, n // (2 * k + 2)) if k else 0
    pairs = [(n - 1 - q * step, q * step) for q in range(k)]
    return F.circle(n, loops=pairs, seed=n + k, radius=n / (2 * np.pi), yaw_bias=1e-5)


def run(ctx, n, k):
    g = graph(n, k)
    ctx.keyframes_reset()
    pts = np.zeros(3, POINT_XYZI)
    for i, e in enumerate(g["poses"]):
        ctx.keyframes_add(np.array((e[3], e[4], e[5], i, e[0], e[1], e[2], 0.0, 2.0 * i), KEYPOSE), pts, pts)
    F.add_to_context(ctx, g["spec"])
    _, r = ctx.pg_optimize()  # warm-up: allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.pg_optimize()
    wall = (time.perf_counter() - t0) / reps
    ctx.set_profiling(True, NAMES)
    before = {q: ctx.kernel_time(q) for q in NAMES}
    ctx.pg_optimize()
    kern = {}
    for q in NAMES:
        ms, cnt = ctx.kernel_time(q)
        kern[q] = {"ms": round(ms - before[q][0], 4), "launches": cnt - before[q][1]}
    ctx.set_profiling(False)
    f = F.model_factors(g["spec"])
    t0 = time.perf_counter()
    _, pi = PM.probe_optimize(f, g["poses"].astype(np.float64))
    cpu = time.perf_counter() - t0
    out = dict(N=n, K=k, optimize_ms=round(wall * 1e3, 3), status=r["status"], lm_steps=r["iterations"], trials=r["trials"],
               pcg_iterations=r["pcg_iterations"], cost_initial=r["cost_initial"], cost_final=r["cost_final"], kernels=kern,
               cpu_probe_ms=round(cpu * 1e3, 3), cpu_probe=dict(status=pi["status"], lm_steps=pi["iterations"],
                                                                 trials=pi["trials"], pcg_iterations=pi["pcg_iterations"],
                                                                 pcg_max=pi["pcg_max"], cost_final=pi["cost_final"]))
    print(json.dumps(out), flush=True)


with api.Context(default_params(16, 1800)) as ctx:
    for n in sizes:
        for k in loops:
            run(ctx, n, k)
    if many > 0:
        run(ctx, max(sizes), many)
