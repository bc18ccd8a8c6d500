"""The pose graph's direct solve and robust loop factors (include/fbr.h "direct solve", "robust loop
factors") through the C-ABI on the GPU: the device's minimiser against the NumPy model's
(tests/pg_loops_model.py over tests/pg_model.py) with the bars of tests/test_pose_graph.py, the two
solvers against each other, byte-stable results, the work-space bound, the false-loop fixture with
fbr_pg_loop_weights, the weighted marginals, the parameter checks, the resources, and the default
path left as it was.

Bars (tests/test_pose_graph.py's): cost within 1e-8 relative; relative poses T_0^-1 T_i within
1e-6 m / 1e-7 rad; absolute poses within the same with a tight prior; with the reference's prior node
0 within 1e-3 m of the model's.
"""
import ctypes
import functools

import numpy as np
import pytest

import pg_fixtures as F
import pg_loops_model as LM
import pg_marg_model as MM
import pg_model as PM
import test_resources as TR
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_PG_CONVERGED, FBR_PG_ITERATIONS, default_params,
                                                                pg_params)
from test_pose_graph import load, result_bytes

TIGHT = LM.TIGHT

# graph: what it exercises (M = 6 K columns of U^T, rows of the dense factor)
GRAPHS = {
    "n5_k0": lambda: F.wrong_chain(5),                                        # M = 0: the step is y
    "n5_k2": lambda: F.circle(5, loops=[(4, 0), (0, 3)], seed=31),            # M = 12, less than a panel
    "n33_k3": lambda: F.circle(33, loops=[(32, 0), (20, 5), (7, 9)], seed=32),  # M = 18
    "n64_k6": lambda: LM.loop_circle(64, 6, seed=33, prior="tight"),          # M = 36, across the 32-column panel
    "n65_k3": lambda: F.circle(65, loops=[(64, 0), (40, 38), (64, 0)], seed=12),  # a pair twice; a loop two nodes apart
    "n64_k8": lambda: LM.loop_circle(64, 8, seed=34),                         # M = 48, exactly one chunk
    # M = 258: past 256 threads, several chunks and panels, nodes past the one-workgroup tail
    "n257_k43": lambda: LM.loop_circle(257, 43, seed=35, prior="tight"),
}


@functools.lru_cache(maxsize=None)
def graph_and_model(name):
    g = GRAPHS[name]()
    return g, F.run_model(g, **TIGHT)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(default_params(16, 1800)) as c:
        yield c


def check_against_model(g, eul, r, R, t, mi):
    d = F.compare(g, eul, R, t)
    dc = abs(r["cost_final"] - mi["cost_final"]) / mi["cost_final"]
    print(f"model {mi['iterations']} steps / {mi['trials']} trials, cost {mi['cost_initial']:.6g} -> {mi['cost_final']:.12g}; "
          f"device {r['iterations']} / {r['trials']}, {r['pcg_iterations']} PCG; cost diff {dc:.2e}; rel {d['rel_t']:.2e} m "
          f"{d['rel_r']:.2e} rad; abs {d['abs_t']:.2e} m {d['abs_r']:.2e} rad; node 0 {d['node0']:.2e} m")
    assert r["status"] in (FBR_PG_CONVERGED, FBR_PG_ITERATIONS)
    assert abs(r["cost_initial"] - mi["cost_initial"]) <= 1e-9 * mi["cost_initial"]
    assert dc < 1e-8
    assert d["rel_t"] < 1e-6 and d["rel_r"] < 1e-7
    if g["absolute"]:
        assert d["abs_t"] < 1e-6 and d["abs_r"] < 1e-7
    else:
        assert d["node0"] < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_direct_solver_reaches_the_models_minimiser(ctx, name):
    g, (R, t, mi) = graph_and_model(name)
    load(ctx, g)
    eul, r = ctx.pg_optimize(pg_params(solver="direct", **TIGHT))
    assert r["pcg_iterations"] == 0 and r["n_loop_factors"] == F.n_loop_factors(g["spec"])
    assert (r["n_nodes"], r["n_factors"]) == (len(g["poses"]), len(g["spec"]))
    check_against_model(g, eul, r, R, t, mi)
    idx, chi2, w = ctx.pg_loop_weights()
    assert len(idx) == r["n_loop_factors"] and np.all(w == 1.0)


@pytest.mark.gpu
def test_direct_against_pcg_on_the_device(ctx):
    """1,025 nodes, 9 loops, GPS: too large for the dense model, so the two solvers against each other."""
    g = LM.loop_circle(1025, 9, seed=36, gps_every=128)
    load(ctx, g)
    ep, rp = ctx.pg_optimize(pg_params(**TIGHT))
    ed, rd = ctx.pg_optimize(pg_params(solver="direct", **TIGHT))
    Rp, tp = PM.poses_from_euler(ep)
    d = F.compare(g, ed, Rp, tp)
    dc = abs(rd["cost_final"] - rp["cost_final"]) / rp["cost_final"]
    print(f"PCG {rp['iterations']} / {rp['trials']}, {rp['pcg_iterations']} iterations; direct {rd['iterations']} / "
          f"{rd['trials']}; cost diff {dc:.2e}; rel {d['rel_t']:.2e} m {d['rel_r']:.2e} rad; abs {d['abs_t']:.2e} m")
    assert rp["pcg_iterations"] > 0 and rd["pcg_iterations"] == 0
    assert rp["status"] in (FBR_PG_CONVERGED, FBR_PG_ITERATIONS) and rd["status"] in (FBR_PG_CONVERGED, FBR_PG_ITERATIONS)
    assert rd["cost_initial"] == rp["cost_initial"]
    assert dc < 1e-8
    assert d["rel_t"] < 1e-6 and d["rel_r"] < 1e-7 and d["abs_t"] < 1e-6 and d["abs_r"] < 1e-7


@pytest.mark.gpu
def test_same_bytes_and_the_work_space_bound(ctx):
    g, _ = graph_and_model("n257_k43")
    load(ctx, g)
    p = pg_params(solver="direct", robust="huber", robust_scale=1.345)
    e1, r1 = ctx.pg_optimize(p, raw=True)
    w1 = ctx.pg_loop_weights()
    e2, r2 = ctx.pg_optimize(p, raw=True)
    w2 = ctx.pg_loop_weights()
    assert e1.tobytes() == e2.tobytes() and result_bytes(r1) == result_bytes(r2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(w1, w2))
    assert r1.status == FBR_PG_CONVERGED and r1.iterations >= 1
    # W alone is 6 * 258 * 257 doubles = 3.2 MB
    with pytest.raises(api.FbrError) as e:
        ctx.pg_optimize(pg_params(solver="direct", max_work_mb=1))
    assert e.value.status == -4
    e3, r3 = ctx.pg_optimize(pg_params(solver="direct", max_work_mb=16))
    assert r3["status"] == FBR_PG_CONVERGED
    e4, _ = ctx.pg_optimize(pg_params(max_work_mb=1))  # the bound is the direct solver's alone
    assert len(e4) == len(e3)


def false_loop_ids(g):
    loops = [k for k, s in enumerate(g["spec"]) if s[0] == "between" and abs(s[1] - s[2]) != 1]
    return np.array(loops, np.int32), len(LM.TRUE_LOOPS)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pcg", "direct"])
@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_robust_loop_factors(ctx, case, solver):
    kind, k = LM.ROBUST_CASES[case]
    g = LM.false_loop_graph(0)
    f = F.model_factors(g["spec"])
    R, t, mi = LM.false_loop_model(0, case)
    Rc, tc, _ = LM.false_loop_model(0, "clean")
    load(ctx, g)
    eul, r = ctx.pg_optimize(pg_params(solver=solver, robust=case, robust_scale=k, **TIGHT))
    assert r["status"] == FBR_PG_CONVERGED and (r["pcg_iterations"] == 0) == (solver == "direct")
    check_against_model(g, eul, r, R, t, mi)
    Rd, td = PM.poses_from_euler(eul)
    off = LM.distance(Rd, td, Rc, tc)
    idx, chi2, w = ctx.pg_loop_weights()
    loops, n_true = false_loop_ids(g)
    ms, mw, _ = LM.chi2_and_weights(f, Rd, td, kind, k)
    print(f"{case} / {solver}: {off[0]:.4f} m {off[1]:.5f} rad from the clean minimiser; true loops' weights >= "
          f"{w[:n_true].min():.3f}, false <= {w[n_true:].max():.2e}; chi2 diff {np.abs(chi2 / ms[loops] - 1).max():.2e}, "
          f"weight diff {np.abs(w / mw[loops] - 1).max():.2e}")
    assert np.array_equal(idx, loops)
    assert off[0] < 0.2
    assert w[n_true:].max() < 0.05 and w[:n_true].min() > 0.5
    assert np.allclose(chi2, ms[loops], rtol=1e-9, atol=0.0) and np.allclose(w, mw[loops], rtol=1e-9, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pcg", "direct"])
def test_least_squares_on_the_false_loops_and_the_chi_square_report(ctx, solver):
    """Without a robust option the two false loops move the poses metres away, every weight is 1 and
    fbr_pg_loop_weights is a plain chi-square report that shows which loops to drop."""
    g = LM.false_loop_graph(0)
    f = F.model_factors(g["spec"])
    R, t, mi = LM.false_loop_model(0, "plain")
    Rc, tc, _ = LM.false_loop_model(0, "clean")
    load(ctx, g)
    eul, r = ctx.pg_optimize(pg_params(solver=solver, **TIGHT))
    check_against_model(g, eul, r, R, t, mi)
    Rd, td = PM.poses_from_euler(eul)
    off = LM.distance(Rd, td, Rc, tc)
    idx, chi2, w = ctx.pg_loop_weights()
    loops, n_true = false_loop_ids(g)
    ms = LM.chi2_and_weights(f, Rd, td)[0]
    print(f"least squares / {solver}: {off[0]:.3f} m from the clean minimiser; chi2 true <= {chi2[:n_true].max():.3g}, "
          f"false >= {chi2[n_true:].min():.3g}")
    assert off[0] > 1.0
    assert np.array_equal(idx, loops) and np.all(w == 1.0)
    assert np.allclose(chi2, ms[loops], rtol=1e-9, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_marginals_after_a_robust_optimise(ctx, case):
    kind, k = LM.ROBUST_CASES[case]
    g = LM.false_loop_graph(0)
    f = F.model_factors(g["spec"])
    load(ctx, g)
    eul, _ = ctx.pg_optimize(pg_params(solver="direct", robust=case, robust_scale=k, **TIGHT))
    cov, info = ctx.pg_marginals()
    ref, H = LM.dense_marginals(f, eul, kind, k)
    plain, _ = LM.dense_marginals(f, eul)
    err, bar = np.abs(cov - ref).max() / np.abs(ref).max(), MM.bar(H)
    print(f"{case}: weighted marginals against the dense inverse {err:.2e}, bar {bar:.2e}; the unweighted ones are "
          f"{np.abs(plain - ref).max() / np.abs(ref).max():.2e} away")
    assert info["status"] == FBR_PG_CONVERGED
    assert err <= bar
    wanted, xy = ctx.pg_gps_gate(25.0)
    assert xy[0] == cov[-1][3, 3] and xy[1] == cov[-1][4, 4]


@pytest.mark.gpu
def test_default_path_is_left_as_it_was(ctx):
    """The same context, default parameters, before and after robust and direct calls: the same bytes."""
    g = LM.false_loop_graph(1)
    load(ctx, g)
    e1, r1 = ctx.pg_optimize(raw=True)
    c1, _ = ctx.pg_marginals()
    ctx.pg_optimize(pg_params(solver="direct", robust="cauchy", robust_scale=3.0))
    ctx.pg_marginals()
    ctx.pg_optimize(pg_params(robust="huber", robust_scale=1.345))
    e2, r2 = ctx.pg_optimize(raw=True)
    c2, _ = ctx.pg_marginals()
    assert e1.tobytes() == e2.tobytes() and result_bytes(r1) == result_bytes(r2) and c1.tobytes() == c2.tobytes()
    assert r1.pcg_iterations > 0


@pytest.mark.gpu
def test_parameter_checks(ctx):
    g = F.circle(5, loops=[(4, 0)], seed=37)
    load(ctx, g)
    bad = [dict(solver=2), dict(solver=-1), dict(robust=3), dict(robust=-1), dict(max_work_mb=-1)]
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        bad += [dict(robust=1, robust_scale=scale), dict(robust=2, robust_scale=scale)]
    for kw in bad:
        with pytest.raises(api.FbrError) as e:
            ctx.pg_optimize(pg_params(**kw))
        assert e.value.status == -1, kw
    ctx.pg_optimize(pg_params(robust_scale=-1.0))  # the scale is not looked at without a robust option
    # fbr_pg_loop_weights' errors are fbr_pg_poses'
    n = ctypes.c_int64()
    assert api.lib().fbr_pg_loop_weights(ctx._h, None, None, None, 0, ctypes.byref(n)) == -4 and n.value == 1
    assert api.lib().fbr_pg_loop_weights(ctx._h, None, None, None, 1, ctypes.byref(n)) == -1
    with api.Context(default_params(16, 1800)) as other:
        with pytest.raises(api.FbrError) as e:
            other.pg_loop_weights()
        assert e.value.status == -7


LOOPS_LIFE_CYCLE = """
import json
import numpy as np
import sys
sys.path.insert(0, "tests")
import pg_fixtures as F
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params, pg_params
base = api.live_resources()
ctx = api.Context(default_params(16, 1800))
alive = api.live_resources()
grown = []
for n in (20, 600):  # the second graph outgrows every buffer of the first
    g = F.circle(n, loops=[(n - 1, 0), (n // 2, 3)], seed=n)
    ctx.keyframes_reset()
    for k in range(n):
        e = g["poses"][k]
        kp = np.array((e[3], e[4], e[5], k, e[0], e[1], e[2], 0.0, 2.0 * k), KEYPOSE)
        ctx.keyframes_add(kp, np.zeros(3, POINT_XYZI), np.zeros(3, POINT_XYZI))
    F.add_to_context(ctx, g["spec"])
    _, r = ctx.pg_optimize(pg_params(solver="direct", robust="huber", robust_scale=1.345))
    ctx.pg_loop_weights()
    ctx.pg_marginals([n - 1])
    grown.append(api.live_resources())
    assert r["status"] in (0, 1), r
ctx.close()
print(json.dumps(dict(base=base, alive=alive, grown=grown, end=api.live_resources())))
"""


@pytest.mark.gpu
def test_buffers_return_to_baseline():
    """The direct solver's work space comes with the first direct optimise, grows in place with a
    larger graph and goes with the context."""
    r = TR.run_child(LOOPS_LIFE_CYCLE)
    assert r["grown"][0] == r["grown"][1]  # grown, not added to
    assert all(g >= a for g, a in zip(r["grown"][0], r["alive"]))
    assert r["end"] == r["base"]
