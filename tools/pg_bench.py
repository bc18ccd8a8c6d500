"""Measurement of the pose-graph optimiser (fbr_pg_optimize): synthetic keyframe chains of N nodes
with K loop factors, the time per optimise, the Levenberg-Marquardt steps, the PCG iterations and the
per-launcher kernel times (fbr_set_profiling), and the same graphs through the CPU probe's host
solve (tests/native/pg_probe.cpp, one thread) for scale.  There is no pass bar: the table
(profiles/pose_graph.md) is the record.  One JSON line per case.
usage: pg_bench.py [reps] [N,N,...] [K,K,...] [K of the extra many-loops case at the largest N]
       pg_bench.py --marginals [reps]   fbr_pg_marginals (every node) after an optimise, for
           (N, K) = (1000, 0), (1000, 10), (10000, 1), (10000, 200): the call time, the per-launcher
           kernel times and the CPU probe's host driver (tests/native/pg_marg_probe.cpp, one thread)
           at the same poses, with the largest difference between the two
       --solver pcg|direct    fbr_pg_params.solver (default pcg); the direct solver's launchers join the kernel times
       --robust none|huber|cauchy   fbr_pg_params.robust, at the scales 1.345 / 3.0
       --no-cpu               skip the CPU probe's host solve (minutes at N = 10,000 with many loops)"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
from feature_base_pointcloud_registration_amd import api  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params, pg_params  # noqa: E402
import pg_fixtures as F  # noqa: E402
import pg_model as PM  # noqa: E402

MARGINALS = "--marginals" in sys.argv
if MARGINALS:
    sys.argv.remove("--marginals")


def option(name, default):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return v


SOLVER, ROBUST = option("--solver", "pcg"), option("--robust", "none")
NO_CPU = "--no-cpu" in sys.argv
if NO_CPU:
    sys.argv.remove("--no-cpu")
PG = dict(solver=SOLVER, robust=ROBUST, robust_scale={"none": 0.0, "huber": 1.345, "cauchy": 3.0}[ROBUST])
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1000, 10000]
loops = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1, 10]
many = int(sys.argv[4]) if len(sys.argv) > 4 else 200
NAMES = ("pg_linearize", "pg_assemble", "pg_factor", "pg_pcg", "pg_retract")
if SOLVER == "direct":
    NAMES = NAMES[:3] + ("pg_direct_y", "pg_marg_solve", "pg_marg_c", "pg_marg_chol", "pg_direct_z", "pg_direct_subst",
                         "pg_direct_delta", "pg_retract")
MARG_NAMES = ("pg_linearize", "pg_assemble", "pg_factor", "pg_selinv", "pg_marg_solve", "pg_marg_c", "pg_marg_chol",
              "pg_marg_cov")
MARG_CASES = ((1000, 0), (1000, 10), (10000, 1), (10000, 200))


def graph(n, k):
    """A circle of ~1 m steps (2e-3 rad / 0.02 m odometry noise, yaw bias 1e-5 rad per step) with k
    loop factors spread over it: (n - 1, 0) first, the others pair a late node with an early one."""
    step = max(1, n // (2 * k + 2)) if k else 0
    pairs = [(n - 1 - q * step, q * step) for q in range(k)]
    return F.circle(n, loops=pairs, seed=n + k, radius=n / (2 * np.pi), yaw_bias=1e-5)


def fill(ctx, g):
    ctx.keyframes_reset()
    pts = np.zeros(3, POINT_XYZI)
    for i, e in enumerate(g["poses"]):
        ctx.keyframes_add(np.array((e[3], e[4], e[5], i, e[0], e[1], e[2], 0.0, 2.0 * i), KEYPOSE), pts, pts)
    F.add_to_context(ctx, g["spec"])


def run_marginals(ctx, n, k):
    import pg_marg_model as MM
    g = graph(n, k)
    fill(ctx, g)
    eul, r = ctx.pg_optimize()
    cov, info = ctx.pg_marginals()  # warm-up: allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.pg_marginals()
    wall = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    ctx.pg_gps_gate()
    gate = time.perf_counter() - t0
    ctx.set_profiling(True, MARG_NAMES)
    before = {q: ctx.kernel_time(q) for q in MARG_NAMES}
    ctx.pg_marginals()
    kern = {}
    for q in MARG_NAMES:
        ms, cnt = ctx.kernel_time(q)
        kern[q] = {"ms": round(ms - before[q][0], 4), "launches": cnt - before[q][1]}
    ctx.set_profiling(False)
    # the probe's driver alone: the factors are packed and the library is loaded before the clock starts
    pf, e = PM.probe_factors(F.model_factors(g["spec"])), np.ascontiguousarray(eul, np.float64)
    ref, lib = np.zeros((n, 6, 6)), MM.probe()
    t0 = time.perf_counter()
    rc = lib.probe_pg_marginals(n, e.ctypes.data, len(pf), pf.ctypes.data, None, n, 0, ref.ctypes.data)
    cpu = time.perf_counter() - t0
    diff = float(np.abs(cov - ref).max() / np.abs(ref).max()) if rc == 0 and info["status"] == 0 else None
    print(json.dumps(dict(N=n, K=k, marginals_ms=round(wall * 1e3, 3), gate_ms=round(gate * 1e3, 3), status=info["status"],
                          work_bytes=info["work_bytes"], optimize_status=r["status"], kernels=kern,
                          cpu_probe_ms=round(cpu * 1e3, 3), cpu_probe_status=rc, device_vs_probe=diff)), flush=True)


def run(ctx, n, k):
    g = graph(n, k)
    fill(ctx, g)
    _, r = ctx.pg_optimize(pg_params(**PG))  # warm-up: allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.pg_optimize(pg_params(**PG))
    wall = (time.perf_counter() - t0) / reps
    ctx.set_profiling(True, NAMES)
    before = {q: ctx.kernel_time(q) for q in NAMES}
    ctx.pg_optimize(pg_params(**PG))
    kern = {}
    for q in NAMES:
        ms, cnt = ctx.kernel_time(q)
        kern[q] = {"ms": round(ms - before[q][0], 4), "launches": cnt - before[q][1]}
    ctx.set_profiling(False)
    out = dict(N=n, K=k, solver=SOLVER, robust=ROBUST, optimize_ms=round(wall * 1e3, 3), status=r["status"],
               lm_steps=r["iterations"], trials=r["trials"], pcg_iterations=r["pcg_iterations"],
               cost_initial=r["cost_initial"], cost_final=r["cost_final"], kernels=kern)
    if not NO_CPU:  # the probe's PCG optimiser, whatever the device's solver: the scale of one CPU thread
        f = F.model_factors(g["spec"])
        t0 = time.perf_counter()
        _, pi = PM.probe_optimize(f, g["poses"].astype(np.float64))
        out["cpu_probe_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["cpu_probe"] = dict(status=pi["status"], lm_steps=pi["iterations"], trials=pi["trials"],
                                pcg_iterations=pi["pcg_iterations"], pcg_max=pi["pcg_max"], cost_final=pi["cost_final"])
    print(json.dumps(out), flush=True)


with api.Context(default_params(16, 1800)) as ctx:
    if MARGINALS:
        for n, k in MARG_CASES:
            run_marginals(ctx, n, k)
        sys.exit(0)
    for n in sizes:
        for k in loops:
            run(ctx, n, k)
    if many > 0:
        run(ctx, max(sizes), many)
