"""NumPy float64 model of include/fbr.h's "robust loop factors" and "direct solve" over the pose-graph
model (tests/pg_model.py, imported unchanged): the robust cost and weights, the weighted dense
Levenberg-Marquardt, a dense Woodbury step, the weighted dense marginals, the false-loop fixture of
the tests (tests/test_pg_loops_model.py on the CPU, tests/test_pose_graph_loops.py on the GPU) and
the CPU probe (tests/native/pg_loops_probe.cpp over csrc/fbr_pg_host.h).
"""
import ctypes
import functools

import numpy as np

import pg_fixtures as F
import pg_marg_model as MM
import pg_model as PM

NONE, HUBER, CAUCHY = 0, 1, 2
KINDS = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY}
TIGHT = dict(rel_cost_tol=1e-12, abs_cost_tol=1e-12, max_iterations=60)


def is_loop(f):
    return f["type"] == "between" and abs(f["i"] - f["j"]) != 1


def robust(kind, k, s):
    """(rho, w) of a factor with s = |r|^2: the contract's Huber and Cauchy; none: (s / 2, 1)."""
    if kind == HUBER:
        e = np.sqrt(s)
        return (0.5 * s, 1.0) if e <= k else (k * (e - 0.5 * k), k / e)
    if kind == CAUCHY:
        return 0.5 * k * k * np.log1p(s / (k * k)), 1.0 / (1.0 + s / (k * k))
    return 0.5 * s, 1.0


def chi2_and_weights(factors, R, t, kind=NONE, k=0.0):
    """Per factor: s = |r|^2 [F], w [F] (1 for every factor that is no loop), rho [F]."""
    s, w, rho = np.zeros(len(factors)), np.ones(len(factors)), np.zeros(len(factors))
    for n, f in enumerate(factors):
        r = PM.residual(f, R[f["i"]], t[f["i"]], *PM._pose_j(f, R, t), jac=False)[0]
        s[n] = float(r @ r)
        rho[n], w[n] = robust(kind, k, s[n]) if is_loop(f) else (0.5 * s[n], 1.0)
    return s, w, rho


def cost(factors, R, t, kind=NONE, k=0.0):
    return float(np.sum(chi2_and_weights(factors, R, t, kind, k)[2]))


def normal_equations(factors, R, t, kind=NONE, k=0.0):
    """Dense H = J^T J and g = J^T r of the factors linearised as sqrt(w) r, sqrt(w) J."""
    n = len(R)
    H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for f in factors:
        i, j = f["i"], f["j"]
        r, Ji, Jj = PM.residual(f, R[i], t[i], *PM._pose_j(f, R, t))
        if is_loop(f):
            sw = np.sqrt(robust(kind, k, float(r @ r))[1])
            r, Ji, Jj = sw * r, sw * Ji, sw * Jj
        si = slice(6 * i, 6 * i + 6)
        H[si, si] += Ji.T @ Ji
        g[si] += Ji.T @ r
        if j >= 0:
            sj = slice(6 * j, 6 * j + 6)
            H[sj, sj] += Jj.T @ Jj
            H[si, sj] += Ji.T @ Jj
            H[sj, si] += Jj.T @ Ji
            g[sj] += Jj.T @ r
    return H, g


def split(factors, R, t, kind=NONE, k=0.0):
    """(T0, U, g): the block-tridiagonal part's undamped normal matrix, the loop factors' weighted
    Jacobians [6K, 6N] and the whole gradient."""
    n = len(R)
    T0, _ = normal_equations([f for f in factors if not is_loop(f)], R, t)
    _, g = normal_equations(factors, R, t, kind, k)
    rows = []
    for f in factors:
        if is_loop(f):
            r, Ji, Jj = PM.residual(f, R[f["i"]], t[f["i"]], R[f["j"]], t[f["j"]])
            sw = np.sqrt(robust(kind, k, float(r @ r))[1])
            u = np.zeros((6, 6 * n))
            u[:, 6 * f["i"]:6 * f["i"] + 6] = sw * Ji
            u[:, 6 * f["j"]:6 * f["j"] + 6] = sw * Jj
            rows.append(u)
    return T0, (np.concatenate(rows) if rows else np.zeros((0, 6 * n))), g


def woodbury_parts(factors, R, t, lam, kind=NONE, k=0.0):
    """The dense Woodbury step of the damped system: dict of y, W, s, delta, H_lam, g."""
    T0, U, g = split(factors, R, t, kind, k)
    H = T0 + U.T @ U
    Hl = H + lam * np.diag(np.diag(H))
    Tl = Hl - U.T @ U
    y = np.linalg.solve(Tl, -g)
    if len(U) == 0:
        return dict(y=y, W=np.zeros((len(g), 0)), s=np.zeros(0), delta=y, H=Hl, g=g)
    W = np.linalg.solve(Tl, U.T)
    s = np.linalg.solve(np.eye(len(U)) + U @ W, U @ y)
    return dict(y=y, W=W, s=s, delta=y - W @ s, H=Hl, g=g)


def lm(factors, R0, t0, kind=NONE, k=0.0, step="dense", **kw):
    """pg_model.lm with the robust cost and the weighted linearisation; step "woodbury": the dense
    Woodbury step in place of numpy.linalg.solve.  Returns (R, t, info)."""
    P = dict(PM.DEFAULTS, **kw)
    R, t = np.array(R0, np.float64), np.array(t0, np.float64)
    n = len(R)
    c = cost(factors, R, t, kind, k)
    info = dict(status=None, iterations=0, trials=0, cost_initial=c, cost_final=c, **{"lambda": P["lambda_init"]})
    lam = P["lambda_init"]
    if c == 0.0:
        info["status"] = PM.CONVERGED
    elif P["max_iterations"] <= 0:
        info["status"] = PM.ITERATIONS
    lin = None
    while info["status"] is None:
        if step == "woodbury":
            d = woodbury_parts(factors, R, t, lam, kind, k)["delta"]
        else:
            if lin is None:
                lin = normal_equations(factors, R, t, kind, k)
            H, g = lin
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        Rn, tn = np.empty_like(R), np.empty_like(t)
        for i in range(n):
            Rn[i], tn[i] = PM.retract(R[i], t[i], d[6 * i:6 * i + 6])
        trial = cost(factors, Rn, tn, kind, k)
        info["trials"] += 1
        if trial < c:
            dec, rel = c - trial, (c - trial) / c
            R, t, c, lin = Rn, tn, trial, None
            info["iterations"] += 1
            lam /= P["lambda_factor"]
            if rel < P["rel_cost_tol"] or dec < P["abs_cost_tol"]:
                info["status"] = PM.CONVERGED
            elif info["iterations"] >= P["max_iterations"]:
                info["status"] = PM.ITERATIONS
        else:
            lam *= P["lambda_factor"]
            if lam > P["lambda_max"]:
                info["status"] = PM.STALLED
    info["cost_final"] = c
    info["lambda"] = lam
    return R, t, info


def dense_marginals(factors, euler, kind=NONE, k=0.0):
    """(Sigma_ii [N, 6, 6], H): the dense inverse of the weighted H at the poses euler [N, 6]."""
    R, t = PM.poses_from_euler(euler)
    H, _ = normal_equations(factors, R, t, kind, k)
    return MM.blocks(np.linalg.inv(H)), H


# ---- graphs with many loops ----
def random_loops(n, count, seed):
    """`count` loop pairs (i, j), |i - j| >= 2, the first one closing the circle."""
    rng = np.random.default_rng(1000 + seed)
    out = [(n - 1, 0)] if count else []
    while len(out) < count:
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if abs(i - j) >= 2:
            out.append((i, j))
    return out


def loop_circle(n, count, seed, **kw):
    return F.circle(n, loops=random_loops(n, count, seed), seed=seed, **kw)


# ---- the false-loop fixture ----
TRUE_LOOPS = [(59, 0), (58, 1), (57, 2), (56, 3)]
FALSE_LOOPS = [(30, 5), (20, 50)]
# (kind, scale): the scales as fbr_pg_params.robust_scale, a float, holds them
ROBUST_CASES = {"huber": (HUBER, float(np.float32(1.345))), "cauchy": (CAUCHY, float(np.float32(3.0)))}


@functools.lru_cache(maxsize=None)
def false_loop_graph(seed, false_loops=True):
    """A 60-node drifting circle, tight prior, four true loops; with false_loops two more whose
    measurement is the identity ("the same place") at the loops' noise."""
    g = F.circle(60, loops=TRUE_LOOPS, prior="tight", seed=seed)
    if false_loops:
        g["spec"] = g["spec"] + [("between", i, j, np.eye(4, dtype=np.float32), F.LOOP_VAR) for i, j in FALSE_LOOPS]
    return g


@functools.lru_cache(maxsize=None)
def false_loop_model(seed, case):
    """(R, t, info) of the model on the fixture: case "clean" (no false loops, least squares), "plain"
    (false loops, least squares), "huber" | "cauchy"."""
    g = false_loop_graph(seed, case != "clean")
    kind, k = ROBUST_CASES.get(case, (NONE, 0.0))
    R0, t0 = PM.poses_from_euler(g["poses"].astype(np.float64))
    return lm(F.model_factors(g["spec"]), R0, t0, kind, k, **TIGHT)


def distance(Ra, ta, Rb, tb):
    """(m, rad) between two sets of absolute poses (the fixture's prior is tight)."""
    return PM.pose_differences(Ra, ta, Rb, tb)


# ---- the CPU probe ----
_PROBE = None


def probe():
    global _PROBE
    if _PROBE is None:
        import conftest
        L = conftest.build_probe("pg_loops_probe")
        assert L.probe_pg_loops_factor_bytes() == PM.PG_FACTOR.itemsize
        VP, I64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
        L.probe_pg_robust.argtypes = [I, D, D, VP, VP]
        L.probe_pg_robust.restype = None
        L.probe_pg_direct_optimize.argtypes = [I64, VP, I64, VP, VP, I, I, D, VP, VP, VP, VP]
        L.probe_pg_direct_step.argtypes = [I64, VP, I64, VP, D, I, I, D, VP]
        L.probe_pg_direct_system.argtypes = [I64, VP, I64, VP, D, I, D, VP, VP, VP]
        L.probe_pg_marginals_robust.argtypes = [I64, VP, I64, VP, I, I, D, VP]
        _PROBE = L
    return _PROBE


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def probe_robust(kind, k, s):
    rho, w = ctypes.c_double(), ctypes.c_double()
    probe().probe_pg_robust(kind, float(k), float(s), ctypes.byref(rho), ctypes.byref(w))
    return rho.value, w.value


def probe_direct_optimize(factors, euler0, kind=NONE, k=0.0, rhs_chunk=0, **kw):
    """The host LM with the direct solve: (poses [N, 6], info dict, chi2 [F], w [F])."""
    P = dict(PM.DEFAULTS, **kw)
    par = np.array([P[n] for n in ("max_iterations", "rel_cost_tol", "abs_cost_tol", "lambda_init", "lambda_factor",
                                   "lambda_max")], np.float64)
    e = np.ascontiguousarray(euler0, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    out, info, chi2, w = np.zeros_like(e), np.zeros(6), np.zeros(len(pf)), np.zeros(len(pf))
    rc = probe().probe_pg_direct_optimize(len(e), _p(e), len(pf), _p(pf), _p(par), int(rhs_chunk), int(kind), float(k),
                                          _p(out), _p(info), _p(chi2), _p(w))
    assert rc == 0, "a node without a factor"
    return out, dict(status=int(info[0]), iterations=int(info[1]), trials=int(info[2]), cost_initial=info[3],
                     cost_final=info[4], **{"lambda": info[5]}), chi2, w


def probe_direct_step(factors, euler, lam, kind=NONE, k=0.0, rhs_chunk=0):
    """(status, delta [6 N]) of one direct step of the damped system at the poses euler."""
    e = np.ascontiguousarray(euler, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    d = np.zeros(6 * len(e))
    rc = probe().probe_pg_direct_step(len(e), _p(e), len(pf), _p(pf), float(lam), int(rhs_chunk), int(kind), float(k), _p(d))
    return rc, d


def probe_direct_system(factors, euler, lam, kind=NONE, k=0.0):
    """(status, delta [6 N], H_lam [6 N, 6 N], g [6 N]): one direct step and the damped system it
    solved, from the probe's own linearisation and assembled blocks."""
    e = np.ascontiguousarray(euler, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    N = 6 * len(e)
    d, H, g = np.zeros(N), np.zeros((N, N)), np.zeros(N)
    rc = probe().probe_pg_direct_system(len(e), _p(e), len(pf), _p(pf), float(lam), int(kind), float(k), _p(d), _p(H), _p(g))
    return rc, d, H, g


def probe_marginals(factors, euler, kind=NONE, k=0.0, rhs_chunk=0):
    """(status, cov [N, 6, 6]) of the host marginals with the loop factors' weights at the poses."""
    e = np.ascontiguousarray(euler, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    cov = np.full((len(e), 6, 6), np.nan)
    rc = probe().probe_pg_marginals_robust(len(e), _p(e), len(pf), _p(pf), int(rhs_chunk), int(kind), float(k), _p(cov))
    return rc, cov
