"""NumPy float64 model of the marginal covariances of include/fbr.h ("marginal covariances"), the
fixtures of their tests (tests/test_pg_marginals_model.py on the CPU, tests/test_pg_marginals.py on
the GPU) and the CPU probe (tests/native/pg_marg_probe.cpp over csrc/fbr_pg_host.h).

Two routes to the 6x6 diagonal blocks of H^-1, H = J^T J undamped at given poses:
  dense_marginals     numpy.linalg.inv of pg_model.normal_equations: the arbiter;
  selinv_marginals    the contract's route restated: selected inversion of the block-tridiagonal part
                      through the cyclic-reduction levels, then the loops by Woodbury.
"""
import ctypes
import functools

import numpy as np

import pg_fixtures as F
import pg_model as PM

TIGHT = dict(rel_cost_tol=1e-12, abs_cost_tol=1e-12, max_iterations=60)
U53, FLOOR = 2.0 ** -53, 2.0 ** -40

# 12 loops; (39, 0) and (0, 39) are the same pair in both directions.  6 K = 72 = two panels of 32
# columns of the dense factor and a remainder of 8.
LOOPS_40 = [(39, 0), (0, 39), (38, 1), (37, 2), (36, 3), (30, 10), (29, 9), (25, 5), (5, 25), (20, 0), (35, 15), (12, 31)]

FIXTURES = {
    "n1": lambda: F.circle(1, prior="tight", seed=21),
    "n2": lambda: F.circle(2, prior="tight", seed=22),
    "n3_k1": lambda: F.circle(3, loops=[(2, 0)], prior="tight", seed=23),
    "n5_k2": lambda: F.circle(5, loops=[(4, 0), (0, 3)], prior="tight", seed=24),
    "n33_k3": lambda: F.circle(33, loops=[(32, 0), (20, 5), (7, 9)], prior="tight", seed=25),
    "n40_k12_gps": lambda: F.circle(40, loops=LOOPS_40, gps_every=8, seed=26),
    "n300_k2_gps": lambda: F.circle(300, loops=[(299, 0), (150, 20)], gps_every=50, seed=27),
}
GATE_FIXTURES = {  # name: (graph, wanted)
    "wanted": (lambda: F.circle(40, loops=[(39, 0)]), 1),
    "not_wanted": (lambda: F.circle(60, loops=[(59, 0), (45, 10), (30, 2)], gps_every=10), 0),
}


def bar(H):
    """The accuracy bar: max |Sigma_ii - model| / max |model| <= max(64 cond(H) 2^-53, 2^-40)."""
    return max(64.0 * np.linalg.cond(H) * U53, FLOOR)


def blocks(S):
    n = len(S) // 6
    return np.stack([S[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n)])


def dense_marginals(factors, euler):
    """(Sigma_ii [N, 6, 6], H) by a dense inverse at the poses euler [N, 6]."""
    R, t = PM.poses_from_euler(euler)
    H, _ = PM.normal_equations(factors, R, t)
    return blocks(np.linalg.inv(H)), H


def _is_loop(f):
    return f["type"] == "between" and abs(f["i"] - f["j"]) != 1


def selinv_marginals(factors, euler):
    """The contract's route in NumPy: T0 = the factors that are no loops, factored by block cyclic
    reduction; P, Q walked up the levels; W = T0^-1 U^T; C = I + U W = Lc Lc^T; Y = Lc^-1 W^T."""
    R, t = PM.poses_from_euler(euler)
    n = len(R)
    T0, _ = PM.normal_equations([f for f in factors if not _is_loop(f)], R, t)
    rows = []
    for f in factors:
        if _is_loop(f):
            _, Ji, Jj = PM.residual(f, R[f["i"]], t[f["i"]], R[f["j"]], t[f["j"]])
            u = np.zeros((6, 6 * n))
            u[:, 6 * f["i"]:6 * f["i"] + 6] = Ji
            u[:, 6 * f["j"]:6 * f["j"] + 6] = Jj
            rows.append(u)
    # the levels: D[m], A[m] = T[m][m-1]; G, H and D^-1 of the eliminated nodes
    D = [T0[6 * m:6 * m + 6, 6 * m:6 * m + 6].copy() for m in range(n)]
    A = [T0[6 * m:6 * m + 6, 6 * m - 6:6 * m].copy() if m else np.zeros((6, 6)) for m in range(n)]
    levels = []
    while True:
        ln = len(D)
        Di, G, Hh = {}, {}, {}
        for k in range(ln):
            if (k & 1) or ln == 1:
                Di[k] = np.linalg.inv(D[k])
                G[k] = Di[k] @ A[k] if k >= 1 else np.zeros((6, 6))
                Hh[k] = Di[k] @ A[k + 1].T if k + 1 < ln else np.zeros((6, 6))
        levels.append((ln, Di, G, Hh))
        if ln == 1:
            break
        nD, nA = [], []
        for q in range((ln + 1) // 2):
            m = 2 * q
            d, a = D[m].copy(), np.zeros((6, 6))
            if m >= 1:
                d -= A[m] @ Hh[m - 1]
                a = -A[m] @ G[m - 1]
            if m + 1 < ln:
                d -= A[m + 1].T @ G[m + 1]
            nD.append(d)
            nA.append(a)
        D, A = nD, nA
    P, Q = [levels[-1][1][0]], [None]
    for ln, Di, G, Hh in reversed(levels[:-1]):
        nP, nQ = P, Q
        P, Q = [None] * ln, [None] * ln
        for m in range(0, ln, 2):
            P[m] = nP[m // 2]
        for k in range(1, ln, 2):
            a = (k - 1) // 2
            right = k + 1 < ln
            Kl = -G[k] @ nP[a]
            Kr = np.zeros((6, 6))
            if right:
                Kl = Kl - Hh[k] @ nQ[a + 1]
                Kr = -G[k] @ nQ[a + 1].T - Hh[k] @ nP[a + 1]
            P[k] = Di[k] - Kl @ G[k].T - Kr @ Hh[k].T
            Q[k] = Kl
            if right:
                Q[k + 1] = Kr.T
    P = np.stack(P)
    if not rows:
        return P
    U = np.concatenate(rows)
    W = np.linalg.solve(T0, U.T)
    Lc = np.linalg.cholesky(np.eye(len(U)) + U @ W)
    Y = np.linalg.solve(Lc, W.T)
    return np.stack([P[i] - Y[:, 6 * i:6 * i + 6].T @ Y[:, 6 * i:6 * i + 6] for i in range(n)])


@functools.lru_cache(maxsize=None)
def graph(name):
    """(graph, model factors), built once."""
    g = (FIXTURES[name] if name in FIXTURES else GATE_FIXTURES[name][0])()
    return g, F.model_factors(g["spec"])


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(graph, model factors, the model's minimiser as euler [N, 6]), computed once."""
    g, f = graph(name)
    R, t, _ = F.run_model(g, **(TIGHT if name in FIXTURES else {}))
    e = PM.euler_from_poses(R, t)
    e.setflags(write=False)
    return g, f, e


# ---- the CPU probe ----
_PROBE = None


def probe():
    global _PROBE
    if _PROBE is None:
        import conftest
        L = conftest.build_probe("pg_marg_probe")
        assert L.probe_pg_marg_factor_bytes() == PM.PG_FACTOR.itemsize
        L.probe_pg_marginals.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
        L.probe_pg_gps_gate.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double,
                                        ctypes.c_void_p, ctypes.c_void_p]
        _PROBE = L
    return _PROBE


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def probe_marginals(factors, euler, nodes=None, rhs_chunk=0):
    """(status, cov [n_out, 6, 6]) of csrc/fbr_pg_host.h's driver."""
    e = np.ascontiguousarray(euler, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    idx = None if nodes is None else np.ascontiguousarray(nodes, np.int64)
    n_out = len(e) if idx is None else len(idx)
    cov = np.full((n_out, 6, 6), np.nan)
    rc = probe().probe_pg_marginals(len(e), _p(e), len(pf), _p(pf), None if idx is None else _p(idx), n_out, int(rhs_chunk),
                                    _p(cov))
    return rc, cov


def probe_gps_gate(factors, euler, threshold=25.0):
    """(status, wanted, cov_xy [2])."""
    e = np.ascontiguousarray(euler, np.float64).reshape(-1, 6)
    pf = PM.probe_factors(factors)
    wanted, xy = ctypes.c_int(-1), np.zeros(2)
    rc = probe().probe_pg_gps_gate(len(e), _p(e), len(pf), _p(pf), float(threshold), ctypes.byref(wanted), _p(xy))
    return rc, wanted.value, xy
