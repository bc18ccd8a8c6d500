"""NumPy float64 model of include/fbr.h's pose-graph contract ("pose graph"): the chart, the three
factors with their analytic Jacobians, and Levenberg-Marquardt with a dense numpy.linalg.solve.
It is the arbiter of the device optimiser and of its CPU probe (tests/native/pg_probe.cpp); its own
Jacobians are checked against central differences (tests/test_pg_model.py).

A pose is (R [3, 3], t [3]); a graph's poses are (R [N, 3, 3], t [N, 3]).  A factor is a dict:
  type "prior" | "between" | "gps", i, j (-1 for prior and gps), ZR [3, 3], Zt [3], w [6] = 1 / sigma in
  tangent order [rotation; translation] (gps: w[:3] = 0).
"""
import ctypes
import os

import numpy as np

PRIOR, BETWEEN, GPS = 0, 1, 2
TYPES = {"prior": PRIOR, "between": BETWEEN, "gps": GPS}
CONVERGED, ITERATIONS, STALLED, NUMERICAL, EMPTY = range(5)

DEFAULTS = dict(max_iterations=30, max_pcg_iterations=200, rel_cost_tol=1e-5, abs_cost_tol=1e-5, pcg_rel_tol=1e-8,
                lambda_init=1e-5, lambda_factor=10.0, lambda_max=1e10)


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, np.float64)
    t2 = float(w @ w)
    if t2 < 1e-12:
        a, b = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        t = np.sqrt(t2)
        a, b = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = skew(w)
    return np.eye(3) + a * K + b * (K @ K)


def log_so3(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    s = 0.5 * np.linalg.norm(v)
    t = np.arctan2(s, c)
    if t * t < 1e-12:
        return 0.5 * (1.0 + t * t / 6.0) * v
    if c > -0.99:
        return 0.5 * t / s * v
    S = 0.5 * (R + R.T)  # = c I + (1 - c) a a^T
    p = int(np.argmax(np.diag(S)))
    a = np.zeros(3)
    a[p] = np.sqrt((S[p, p] - c) / (1.0 - c))
    for q in range(3):
        if q != p:
            a[q] = S[p, q] / ((1.0 - c) * a[p])
    a /= np.linalg.norm(a)
    if a @ v < 0.0:
        a = -a
    return t * a


def jr_inv(phi):
    t2 = float(phi @ phi)
    if t2 < 1e-6:
        k = 1.0 / 12.0 + t2 / 720.0
    else:
        t = np.sqrt(t2)
        k = 1.0 / t2 - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    K = skew(phi)
    return np.eye(3) + 0.5 * K + k * (K @ K)


def rot_from_euler(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def poses_from_euler(e):
    """[N, 6] = [roll, pitch, yaw, x, y, z] -> (R [N, 3, 3], t [N, 3])."""
    e = np.asarray(e, np.float64).reshape(-1, 6)
    return np.stack([rot_from_euler(*p[:3]) for p in e]), e[:, 3:].copy()


def euler_from_poses(R, t):
    R = np.asarray(R).reshape(-1, 3, 3)
    out = np.zeros((len(R), 6))
    out[:, 0] = np.arctan2(R[:, 2, 1], R[:, 2, 2])
    out[:, 1] = np.arcsin(np.clip(-R[:, 2, 0], -1.0, 1.0))
    out[:, 2] = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    out[:, 3:] = np.asarray(t).reshape(-1, 3)
    return out


def between_pose(Ra, ta, Rb, tb):
    return Ra.T @ Rb, Ra.T @ (tb - ta)


def retract(R, t, d):
    return R @ exp_so3(d[:3]), t + R @ d[3:]


def make_factor(kind, i, j=-1, ZR=None, Zt=None, var=None):
    w = np.zeros(6)
    var = np.asarray(var, np.float64)
    if kind == "gps":
        w[3:] = 1.0 / np.sqrt(var)
    else:
        w[:] = 1.0 / np.sqrt(var)
    return dict(type=kind, i=int(i), j=int(j), ZR=np.eye(3) if ZR is None else np.asarray(ZR, np.float64),
                Zt=np.asarray(Zt, np.float64), w=w)


def residual(f, Ri, ti, Rj=None, tj=None, jac=True):
    """Whitened residual [6] and Jacobians (Ji, Jj) [6, 6] (Jj zero for prior and gps)."""
    w = f["w"]
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    if f["type"] == "gps":
        r = np.zeros(6)
        r[3:] = ti - f["Zt"]
        Ji[3:, 3:] = Ri
        return r * w, w[:, None] * Ji, Jj
    if f["type"] == "between":
        DR, Dt = between_pose(Ri, ti, Rj, tj)
    else:
        DR, Dt = Ri, ti
    ZR, Zt = f["ZR"], f["Zt"]
    E = ZR.T @ DR
    phi = log_so3(E)
    r = np.concatenate([phi, ZR.T @ (Dt - Zt)])
    if not jac:
        return r * w, None, None
    J = jr_inv(phi)
    Jn = np.zeros((6, 6))
    Jn[:3, :3] = J
    Jn[3:, 3:] = E
    if f["type"] == "prior":
        return r * w, w[:, None] * Jn, Jj
    Ji[:3, :3] = -J @ DR.T
    Ji[3:, :3] = ZR.T @ skew(Dt)
    Ji[3:, 3:] = -ZR.T
    return r * w, w[:, None] * Ji, w[:, None] * Jn


def numeric_jacobians(f, Ri, ti, Rj, tj, h=1e-6):
    """Central differences of the whitened residual in the chart."""
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        a = residual(f, *retract(Ri, ti, d), Rj, tj, jac=False)[0]
        b = residual(f, *retract(Ri, ti, -d), Rj, tj, jac=False)[0]
        Ji[:, k] = (a - b) / (2 * h)
        if f["type"] == "between":
            a = residual(f, Ri, ti, *retract(Rj, tj, d), jac=False)[0]
            b = residual(f, Ri, ti, *retract(Rj, tj, -d), jac=False)[0]
            Jj[:, k] = (a - b) / (2 * h)
    return Ji, Jj


def _pose_j(f, R, t):
    return (R[f["j"]], t[f["j"]]) if f["j"] >= 0 else (None, None)


def cost(factors, R, t):
    c = 0.0
    for f in factors:
        r = residual(f, R[f["i"]], t[f["i"]], *_pose_j(f, R, t), jac=False)[0]
        c += 0.5 * float(r @ r)
    return c


def normal_equations(factors, R, t):
    """Dense H = J^T J [6N, 6N] and g = J^T r [6N]."""
    n = len(R)
    H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for f in factors:
        i, j = f["i"], f["j"]
        r, Ji, Jj = residual(f, R[i], t[i], *_pose_j(f, R, t))
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


def _solve_chain(factors, R, t, lam):
    """(H + lam diag H) d = -g for a graph without off-band factors, by block Thomas elimination
    (what a dense solve computes, without the [6N, 6N] array: the large chains of the GPU tests)."""
    n = len(R)
    D, A, g = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6))
    for f in factors:
        i, j = f["i"], f["j"]
        r, Ji, Jj = residual(f, R[i], t[i], *_pose_j(f, R, t))
        D[i] += Ji.T @ Ji
        g[i] += Ji.T @ r
        if j >= 0:
            assert abs(i - j) == 1
            D[j] += Jj.T @ Jj
            g[j] += Jj.T @ r
            if i > j:
                A[i] += Ji.T @ Jj
            else:
                A[j] += Jj.T @ Ji
    for m in range(n):
        D[m][np.diag_indices(6)] *= 1.0 + lam
    b = -g
    for m in range(1, n):  # forward: eliminate the sub-diagonal
        W = np.linalg.solve(D[m - 1], A[m].T).T  # A[m] D[m-1]^-1
        D[m] = D[m] - W @ A[m].T
        b[m] = b[m] - W @ b[m - 1]
    x = np.zeros((n, 6))
    x[n - 1] = np.linalg.solve(D[n - 1], b[n - 1])
    for m in range(n - 2, -1, -1):
        x[m] = np.linalg.solve(D[m], b[m] - A[m + 1].T @ x[m + 1])
    return x.reshape(-1)


def lm(factors, R0, t0, chain_solver=False, **kw):
    """The contract's Levenberg-Marquardt.  Returns (R, t, info)."""
    P = dict(DEFAULTS, **kw)
    R, t = np.array(R0, np.float64), np.array(t0, np.float64)
    n = len(R)
    c = cost(factors, R, t)
    info = dict(status=None, iterations=0, trials=0, cost_initial=c, cost_final=c, **{"lambda": P["lambda_init"]})
    lam = P["lambda_init"]
    if c == 0.0:
        info["status"] = CONVERGED
    elif P["max_iterations"] <= 0:
        info["status"] = ITERATIONS
    lin = None
    while info["status"] is None:
        if chain_solver:
            d = _solve_chain(factors, R, t, lam)
        else:
            if lin is None:
                lin = normal_equations(factors, R, t)
            H, g = lin
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        Rn, tn = np.empty_like(R), np.empty_like(t)
        for i in range(n):
            Rn[i], tn[i] = retract(R[i], t[i], d[6 * i:6 * i + 6])
        trial = cost(factors, Rn, tn)
        info["trials"] += 1
        if trial < c:
            dec, rel = c - trial, (c - trial) / c
            R, t, c, lin = Rn, tn, trial, None
            info["iterations"] += 1
            lam /= P["lambda_factor"]
            if rel < P["rel_cost_tol"] or dec < P["abs_cost_tol"]:
                info["status"] = CONVERGED
            elif info["iterations"] >= P["max_iterations"]:
                info["status"] = ITERATIONS
        else:
            lam *= P["lambda_factor"]
            if lam > P["lambda_max"]:
                info["status"] = STALLED
    info["cost_final"] = c
    info["lambda"] = lam
    return R, t, info


# ---- comparisons ----
def relative_poses(R, t):
    """T_0^-1 T_i: gauge-invariant under a rigid motion of the whole trajectory."""
    return np.stack([R[0].T @ Ri for Ri in R]), np.stack([R[0].T @ (ti - t[0]) for ti in t])


def pose_differences(Ra, ta, Rb, tb):
    """(max |t_a - t_b|, max rotation angle of R_a^T R_b) over the nodes."""
    dt = float(np.max(np.linalg.norm(np.asarray(ta) - np.asarray(tb), axis=1)))
    dr = max(float(np.linalg.norm(log_so3(A.T @ B))) for A, B in zip(Ra, Rb))
    return dt, dr


# ---- the CPU probe (tests/native/pg_probe.cpp over csrc/fbr_pg.h) ----
PG_FACTOR = np.dtype([("type", "<i4"), ("i", "<i4"), ("j", "<i4"), ("loop", "<i4"), ("Z", "<f8", 12), ("w", "<f8", 6)])
_PROBE = None


def probe():
    global _PROBE
    if _PROBE is None:
        import conftest
        L = conftest.build_probe("pg_probe")
        assert L.probe_pg_factor_bytes() == PG_FACTOR.itemsize
        L.probe_pg_optimize.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
        L.probe_pg_tridiag_solve.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4
        _PROBE = L
    return _PROBE


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def probe_factors(factors):
    out = np.zeros(len(factors), PG_FACTOR)
    for k, f in enumerate(factors):
        out[k]["type"], out[k]["i"], out[k]["j"] = TYPES[f["type"]], f["i"], f["j"]
        out[k]["loop"] = int(f["type"] == "between" and abs(f["i"] - f["j"]) != 1)
        out[k]["Z"][:9] = f["ZR"].reshape(9)
        out[k]["Z"][9:] = f["Zt"]
        out[k]["w"] = f["w"]
    return out


def _pose12(R, t):
    return np.ascontiguousarray(np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]))


def probe_residual(f, Ri, ti, Rj=None, tj=None):
    pf = probe_factors([f])
    Xi = _pose12(Ri, ti)
    Xj = _pose12(Rj, tj) if Rj is not None else np.zeros(12)
    r, Ji, Jj = np.zeros(6), np.zeros(36), np.zeros(36)
    probe().probe_pg_factor(_p(pf), _p(Xi), _p(Xj), _p(r), _p(Ji), _p(Jj))
    return r, Ji.reshape(6, 6), Jj.reshape(6, 6)


def probe_log(R):
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    w = np.zeros(3)
    probe().probe_pg_log(_p(R), _p(w))
    return w


def probe_chol6(A):
    A = np.ascontiguousarray(A, np.float64).reshape(36)
    L = np.zeros(36)
    ok = probe().probe_pg_chol6(_p(A), _p(L))
    return bool(ok), L.reshape(6, 6)


def probe_tridiag_solve(D, A, b):
    D, A, b = (np.ascontiguousarray(v, np.float64) for v in (D, A, b))
    x = np.zeros_like(b)
    ok = probe().probe_pg_tridiag_solve(len(D), _p(D), _p(A), _p(b), _p(x))
    return bool(ok), x


def probe_optimize(factors, euler0, **kw):
    """The probe's host LM + PCG.  Returns (poses [N, 6], info dict)."""
    P = dict(DEFAULTS, **kw)
    par = np.array([P[k] for k in ("max_iterations", "max_pcg_iterations", "rel_cost_tol", "abs_cost_tol", "pcg_rel_tol",
                                   "lambda_init", "lambda_factor", "lambda_max")], np.float64)
    e = np.ascontiguousarray(euler0, np.float64).reshape(-1, 6)
    pf = probe_factors(factors)
    out, info = np.zeros_like(e), np.zeros(8)
    rc = probe().probe_pg_optimize(len(e), _p(e), len(pf), _p(pf), _p(par), _p(out), _p(info))
    assert rc == 0, "a node without a factor"
    return out, dict(status=int(info[0]), iterations=int(info[1]), trials=int(info[2]), pcg_iterations=int(info[3]),
                     cost_initial=info[4], cost_final=info[5], pcg_max=int(info[7]), **{"lambda": info[6]})
