"""The pose graph's direct solve and robust loop factors on the CPU: the CPU build of the kernels'
arithmetic (tests/native/pg_loops_probe.cpp over csrc/fbr_pg_host.h and csrc/fbr_pg.h) against the
NumPy model (tests/pg_loops_model.py over tests/pg_model.py).  No GPU is needed.

Bars.  The optimiser's are tests/test_pg_model.py's: cost within 1e-8 relative, relative poses within
1e-6 m / 1e-7 rad, node 0 within 1e-3 m under the reference prior.  The direct step's residual bar
is derived in test_direct_step_residual.  Each test prints the figures it asserts.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import pg_fixtures as F
import pg_loops_model as LM
import pg_marg_model as MM
import pg_model as PM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = LM.TIGHT

# (nodes, loops): K = 0, 1, 2 and 6 (6 K = 36 crosses the dense factor's 32-column panel) on 40 nodes,
# K = 43 (258 columns: several panels and chunks) on 90
STEP_GRAPHS = [(40, 0), (40, 1), (40, 2), (40, 6), (90, 43)]


def graph(n, K, prior):
    g = LM.loop_circle(n, K, seed=40 + K, prior=prior)
    return g, F.model_factors(g["spec"])


def rel_residual(H, g, d):
    return float(np.linalg.norm(H @ d + g) / np.linalg.norm(g))


@pytest.mark.parametrize("lam", [1e-5, 1e-9])
@pytest.mark.parametrize("prior", ["reference", "tight"])
@pytest.mark.parametrize("n,K", STEP_GRAPHS)
def test_direct_step_residual(n, K, prior, lam):
    """|H_lam delta + g| / |g| of the probe's direct step beside the stored poses against that of
    numpy.linalg.solve on the same damped system: the H_lam and g the probe itself assembled (the
    model's differ from them by the rounding of every factor's Jacobians, which neither solve is
    answerable for; the model's system is compared with it below).

    The bar is the dense solve's own residual times a margin.  The direct step's residual is
    r_y - R_W s + U^T r_C: the residuals of y = T^-1 (-g), of W = T^-1 U^T (times s) and of the solve
    with C, three solves where the dense route has one, the first two through the ceil(log2 N) + 1
    levels of the cyclic reduction; and they scale with |y| and |W s|, the two terms whose difference
    is delta, where the dense solve's scales with |delta|.  So
        margin = 3 (ceil(log2 N) + 1) max(1, (|y| + |W s|) / |delta|),
    with y, W s and delta from the model's dense Woodbury step: a property of the system, not of the
    probe.

    Measured, over both priors and both lambdas: K <= 6: probe <= 1.2e-15, dense solve <= 6.7e-16,
    bars 4.1e-15 .. 3.2e-14; K = 43 (kappa 15 .. 25): probe 6.4e-14 .. 1.4e-13, dense solve 2.5e-15 ..
    3.8e-15, bars 9.9e-13 .. 2.0e-12.  The model's dense Woodbury step leaves 4.8e-15 .. 5.5e-14 on the
    probe's system: its own Jacobians' rounding.
    """
    g, f = graph(n, K, prior)
    # the stored poses satisfy the odometry exactly (K = 0: a zero gradient), so linearise beside them
    sigma = np.array([1e-3, 1e-3, 1e-3, 1e-2, 1e-2, 1e-2])
    e = g["poses"].astype(np.float64) + np.random.default_rng(n + K).normal(0, 1.0, (n, 6)) * sigma
    R, t = PM.poses_from_euler(e)
    w = LM.woodbury_parts(f, R, t, lam)
    rc, d, H, gr = LM.probe_direct_system(f, e, lam)
    assert np.array_equal(H, H.T)
    assert np.abs(H - w["H"]).max() <= 1e-12 * np.abs(H).max() and np.abs(gr - w["g"]).max() <= 1e-9 * np.abs(gr).max()
    dense = np.linalg.solve(H, -gr)
    assert LM.probe_direct_step(f, e, lam)[1].tobytes() == d.tobytes()
    kappa = max(1.0, (np.linalg.norm(w["y"]) + np.linalg.norm(w["W"] @ w["s"])) / np.linalg.norm(w["delta"]))
    margin = 3.0 * (math.ceil(math.log2(n)) + 1) * kappa
    r_probe, r_dense, r_model = rel_residual(H, gr, d), rel_residual(H, gr, dense), rel_residual(H, gr, w["delta"])
    print(f"n {n} K {K} {prior} lambda {lam:g}: probe {r_probe:.2e}, dense solve {r_dense:.2e}, dense Woodbury "
          f"{r_model:.2e}; kappa {kappa:.2e}, margin {margin:.2e}, bar {margin * r_dense:.2e}")
    assert rc == 0
    assert r_probe <= margin * r_dense


def test_direct_step_does_not_depend_on_the_chunk():
    g, f = graph(40, 6, "tight")
    e = g["poses"].astype(np.float64)
    _, ref = LM.probe_direct_step(f, e, 1e-5)
    for chunk in (1, 7, 36):
        rc, d = LM.probe_direct_step(f, e, 1e-5, rhs_chunk=chunk)
        assert rc == 0 and d.tobytes() == ref.tobytes()


@pytest.mark.parametrize("prior", ["reference", "tight"])
@pytest.mark.parametrize("n,K", STEP_GRAPHS)
def test_probe_direct_lm_reaches_the_models_minimiser(n, K, prior):
    # (without a loop the circle's stored poses are the minimum already: the chain that disagrees with itself)
    g, f = graph(n, K, prior) if K else (lambda c: (c, F.model_factors(c["spec"])))(F.wrong_chain(n, prior=prior))
    R, t, mi = F.run_model(g, **TIGHT)
    eul, info, chi2, w = LM.probe_direct_optimize(f, g["poses"].astype(np.float64), **TIGHT)
    d = F.compare(g, eul, R, t)
    dc = abs(info["cost_final"] - mi["cost_final"]) / mi["cost_final"]
    print(f"n {n} K {K} {prior}: model {mi['iterations']} steps / {mi['trials']} trials, probe {info['iterations']} / "
          f"{info['trials']}; cost diff {dc:.2e}; rel {d['rel_t']:.2e} m {d['rel_r']:.2e} rad; abs {d['abs_t']:.2e} m; "
          f"node 0 {d['node0']:.2e} m")
    assert info["status"] in (PM.CONVERGED, PM.ITERATIONS)
    assert dc < 1e-8
    assert d["rel_t"] < 1e-6 and d["rel_r"] < 1e-7
    if g["absolute"]:
        assert d["abs_t"] < 1e-6 and d["abs_r"] < 1e-7
    else:
        assert d["node0"] < 1e-3
    assert np.all(w == 1.0)
    Rp, tp = PM.poses_from_euler(eul)
    s_model = LM.chi2_and_weights(f, Rp, tp)[0]
    assert np.allclose(chi2, s_model, rtol=1e-9, atol=1e-18)


def test_model_woodbury_lm_is_the_dense_lm():
    """The model's own two routes: the dense Woodbury step drives LM to the dense LM's minimiser."""
    g, f = graph(40, 6, "tight")
    R0, t0 = PM.poses_from_euler(g["poses"].astype(np.float64))
    Ra, ta, ia = LM.lm(f, R0, t0, **TIGHT)
    Rb, tb, ib = LM.lm(f, R0, t0, step="woodbury", **TIGHT)
    dt, dr = PM.pose_differences(Ra, ta, Rb, tb)
    print(f"dense {ia['iterations']}/{ia['trials']}, woodbury {ib['iterations']}/{ib['trials']}; {dt:.2e} m {dr:.2e} rad")
    assert abs(ia["cost_final"] - ib["cost_final"]) < 1e-8 * ia["cost_final"]
    assert dt < 1e-6 and dr < 1e-7


# ---- robust ----
def ulp_neighbours(k):
    return [0.0, np.nextafter(k, 0.0), k, np.nextafter(k, np.inf), 1e3 * k]


@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_pg_robust_matches_the_model(case):
    kind, k = LM.ROBUST_CASES[case]
    for e in ulp_neighbours(k):
        s = e * e
        rho, w = LM.probe_robust(kind, k, s)
        mr, mw = LM.robust(kind, k, s)
        assert abs(rho - mr) <= 4e-16 * abs(mr) and abs(w - mw) <= 4e-16 * abs(mw), (case, e)
    # across the threshold both are continuous
    lo, hi = LM.probe_robust(kind, k, np.nextafter(k, 0.0) ** 2), LM.probe_robust(kind, k, np.nextafter(k, np.inf) ** 2)
    assert abs(lo[0] - hi[0]) <= 1e-14 * hi[0] and abs(lo[1] - hi[1]) <= 1e-14
    assert LM.probe_robust(LM.NONE, 0.0, 7.0) == (3.5, 1.0)


@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_weight_is_twice_the_derivative_of_rho(case):
    """w = 2 rho'(s) by central differences, h = 1e-5 s: truncation ~1e-10 and rounding ~1e-11
    relative; the bar is 1e-8.  The points stay clear of Huber's kink at s = k^2."""
    kind, k = LM.ROBUST_CASES[case]
    for s in (0.01, 0.5 * k * k, 2.0 * k * k, 50.0, 1e4):
        h = 1e-5 * s
        d = (LM.probe_robust(kind, k, s + h)[0] - LM.probe_robust(kind, k, s - h)[0]) / (2.0 * h)
        w = LM.probe_robust(kind, k, s)[1]
        assert abs(2.0 * d - w) <= 1e-8 * w, (case, s, 2.0 * d, w)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_false_loop_fixture(seed):
    """The conditions the fixture has to meet, on the model: least squares is ruined by the two false
    loops, Huber 1.345 and Cauchy 3.0 end at the clean graph's minimiser, the false loops lose their
    weight and the true ones keep it."""
    Rc, tc, _ = LM.false_loop_model(seed, "clean")
    Rp, tp, _ = LM.false_loop_model(seed, "plain")
    off = LM.distance(Rp, tp, Rc, tc)
    print(f"seed {seed}: least squares {off[0]:.3f} m {off[1]:.4f} rad from the clean minimiser")
    assert off[0] > 1.0
    f = F.model_factors(LM.false_loop_graph(seed)["spec"])
    loops = [n for n, x in enumerate(f) if LM.is_loop(x)]
    for case, (kind, k) in LM.ROBUST_CASES.items():
        R, t, info = LM.false_loop_model(seed, case)
        d = LM.distance(R, t, Rc, tc)
        _, w, _ = LM.chi2_and_weights(f, R, t, kind, k)
        true_w, false_w = w[loops[:4]], w[loops[4:]]
        print(f"seed {seed} {case}: {d[0]:.4f} m {d[1]:.5f} rad; true loops' weights >= {true_w.min():.3f}, false "
              f"<= {false_w.max():.2e}; {info['iterations']} steps")
        assert info["status"] == PM.CONVERGED
        assert d[0] < 0.2
        assert false_w.max() < 0.05 and true_w.min() > 0.5


@pytest.mark.parametrize("solver_chunk", [0, 7])
@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_probe_robust_lm_reaches_the_models_minimiser(case, solver_chunk):
    kind, k = LM.ROBUST_CASES[case]
    g = LM.false_loop_graph(0)
    f = F.model_factors(g["spec"])
    R, t, mi = LM.false_loop_model(0, case)
    eul, info, chi2, w = LM.probe_direct_optimize(f, g["poses"].astype(np.float64), kind, k, rhs_chunk=solver_chunk, **TIGHT)
    d = F.compare(g, eul, R, t)
    dc = abs(info["cost_final"] - mi["cost_final"]) / mi["cost_final"]
    ms, mw, _ = LM.chi2_and_weights(f, R, t, kind, k)
    print(f"{case}: model {mi['iterations']}/{mi['trials']}, probe {info['iterations']}/{info['trials']}; cost diff "
          f"{dc:.2e}; abs {d['abs_t']:.2e} m {d['abs_r']:.2e} rad")
    assert info["status"] == PM.CONVERGED
    assert abs(info["cost_initial"] - mi["cost_initial"]) <= 1e-9 * mi["cost_initial"]
    assert dc < 1e-8
    assert d["abs_t"] < 1e-6 and d["abs_r"] < 1e-7
    assert np.allclose(chi2, ms, rtol=1e-9, atol=1e-18) and np.allclose(w, mw, rtol=1e-9)


@pytest.mark.parametrize("case", list(LM.ROBUST_CASES))
def test_weighted_marginals(case):
    """The host marginals with the loop factors' weights against the dense inverse of the weighted
    H, under the marginals' own bar; and they differ from the unweighted ones."""
    kind, k = LM.ROBUST_CASES[case]
    f = F.model_factors(LM.false_loop_graph(0)["spec"])
    R, t, _ = LM.false_loop_model(0, case)
    e = PM.euler_from_poses(R, t)
    ref, H = LM.dense_marginals(f, e, kind, k)
    rc, cov = LM.probe_marginals(f, e, kind, k)
    err, bar = np.abs(cov - ref).max() / np.abs(ref).max(), MM.bar(H)
    plain, _ = LM.dense_marginals(f, e)
    print(f"{case}: weighted marginals against the dense inverse {err:.2e}, bar {bar:.2e}; the unweighted ones differ "
          f"by {np.abs(plain - ref).max() / np.abs(ref).max():.2e}")
    assert rc == PM.CONVERGED
    assert err <= bar
    assert np.abs(plain - ref).max() > 1e3 * bar * np.abs(ref).max()
    rc, cov7 = LM.probe_marginals(f, e, kind, k, rhs_chunk=7)
    assert rc == PM.CONVERGED and cov7.tobytes() == cov.tobytes()


def test_singular_system_is_numerical():
    """A T_lambda that is not positive definite: the step reports a bad pivot, and the optimiser
    built on it ends with FBR_PG_NUMERICAL at the stored poses.  The damping is -2 (the C-ABI refuses
    it; the probe does not), which makes T's diagonal negative whatever the rounding: a singular T's
    last pivot is rounding noise of either sign.  Through the probe only; the device is not made to
    fail on purpose."""
    g = F.circle(12, loops=[(11, 0)], seed=28, no_prior=True)
    f = F.model_factors(g["spec"])
    e = g["poses"].astype(np.float64)
    rc, _ = LM.probe_direct_step(f, e, -2.0)
    assert rc == PM.NUMERICAL
    eul, info, _, w = LM.probe_direct_optimize(f, e, lambda_init=-2.0)
    assert info["status"] == PM.NUMERICAL and info["trials"] == 1 and np.array_equal(eul, e) and np.all(w == 1.0)


def test_params_mirror_and_validation_constants():
    from feature_base_pointcloud_registration_amd import api
    from feature_base_pointcloud_registration_amd.fbr_types import FbrPgParams, pg_params
    assert ctypes.sizeof(FbrPgParams) == 72
    assert (FbrPgParams.solver.offset, FbrPgParams.robust.offset, FbrPgParams.robust_scale.offset,
            FbrPgParams.max_work_mb.offset) == (56, 60, 64, 68)
    p = pg_params(solver="direct", robust="cauchy", robust_scale=3.0, max_work_mb=64)
    assert (p.solver, p.robust, p.robust_scale, p.max_work_mb) == (1, 2, 3.0, 64)
    d = FbrPgParams()
    api.lib().fbr_pg_params_default(ctypes.byref(d))
    assert (d.solver, d.robust, d.robust_scale, d.max_work_mb) == (0, 0, 0.0, 0)
    assert "fbr_pg_loop_weights" in api.EXPORTED_SYMBOLS and callable(api.Context.pg_loop_weights)
    src = open(os.path.join(REPO, "include", "fbr.h")).read()
    for name, v in (("FBR_PG_SOLVER_PCG", 0), ("FBR_PG_SOLVER_DIRECT", 1), ("FBR_PG_ROBUST_NONE", 0),
                    ("FBR_PG_ROBUST_HUBER", 1), ("FBR_PG_ROBUST_CAUCHY", 2)):
        assert f"#define {name} {v}\n" in src


def test_host_driver_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into Python, never run on a GPU) runs the
    direct LM's host driver under AddressSanitizer and UBSan: K = 0, 2 and 6, rhs_chunk 7 and 1, both
    robust kinds, the weighted marginals, a singular T, a single node."""
    exe = str(tmp_path / "pg_loops_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(REPO, "feature_base_pointcloud_registration_amd", "csrc"),
                           "-o", exe, os.path.join(REPO, "tests", "native", "pg_loops_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pg_loops_check ok" in r.stdout
