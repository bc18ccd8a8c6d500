"""Clouds with known correspondences, the float64 reference and the bars for the tests of the ICP's
transformation estimate (tests/test_icp_solve.py on the CPU, tests/test_icp_step.py on the GPU).
TEST INFRASTRUCTURE ONLY.

Reference: Umeyama without scaling on centred float64 coordinates with S = diag(1, 1, det(U) det(V)),
rounded to float32.  The code under test works from uncentred float64 sums of the same float32
points, so only the final rounding differs (and, for a cloud far from the origin, the cancellation
in sigma = E[t s^T] - mt ms^T, which the bars below still have to cover).

Bars (every case): det R > 0; |R R^T - I| <= 1e-6 (float entries, 6e-8 rounding each).
Where the rotation is unique (w1 / w0 >= 0.1, asserted on the inputs): R within 2 float32 ulps at
1.0 of the reference, t within 2 ulps at max(1, |t_ref|) (per component).
Otherwise (a line, coincident points): T maps every source point onto its target within
1e-5 (1 + max |coordinate|).
"""
import numpy as np

F32 = np.float32
ULP1 = float(np.spacing(F32(1.0)))  # 2^-23


def rot(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis` (float64)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_rot(rng, max_angle):
    return rot(rng.normal(size=3), rng.uniform(-max_angle, max_angle))


def move(points, R, t, centre=None):
    """R (p - c) + c + t in float64, rounded to float32."""
    p = np.asarray(points, np.float64)
    c = p.mean(0) if centre is None else np.asarray(centre, np.float64)
    return ((p - c) @ R.T + c + t).astype(F32)


def sums17(s, t):
    """count, sum s, sum t, sum t_r s_c (row-major), sum d2 (unused by the solve: 0) in float64 from
    float32 points, as k_icp_reduce takes them."""
    s, t = np.asarray(s, F32).astype(np.float64), np.asarray(t, F32).astype(np.float64)
    return np.concatenate([[len(s)], s.sum(0), t.sum(0), (t[:, :, None] * s[:, None, :]).sum(0).ravel(), [0.0]])


def reference(s, t):
    """(R, tr, w) in float64: centred Umeyama with the det(U) det(V) rule; w the singular values."""
    s, t = np.asarray(s, F32).astype(np.float64), np.asarray(t, F32).astype(np.float64)
    ms, mt = s.mean(0), t.mean(0)
    U, w, Vt = np.linalg.svd((t - mt).T @ (s - ms) / len(s))
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    return R, mt - R @ ms, w


def check(T, s, t, unique, ref=None):
    """The bars of the module docstring on a 3x4 (or 4x4) float32 T; returns a list of failures
    (empty = pass), so a caller can count draws.  `ref`: a float32 T to compare with instead of
    reference()'s (tests/loop_model.py's, which is the same computation)."""
    T = np.asarray(T, F32).reshape(-1, 4)[:3]
    s, t = np.asarray(s, F32), np.asarray(t, F32)
    R, tr = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    bad = []
    if not np.linalg.det(R) > 0:
        bad.append("det R = %.3g" % np.linalg.det(R))
    orth = np.abs(R @ R.T - np.eye(3)).max()
    if not orth <= 1e-6:
        bad.append("|R R^T - I| = %.3g" % orth)
    Rr, tref, w = reference(s, t)
    if ref is not None:
        ref = np.asarray(ref, F32).reshape(-1, 4)[:3]
        Rr, tref = ref[:, :3].astype(np.float64), ref[:, 3].astype(np.float64)
    if unique:
        assert w[1] / w[0] >= 0.1, w  # a condition on the input
        dR = np.abs(R - Rr.astype(F32).astype(np.float64)).max()
        if not dR <= 2 * ULP1:
            bad.append("|R - R_ref| = %.3g" % dR)
        t32 = tref.astype(F32)
        tol = 2 * np.spacing(np.maximum(np.abs(t32), F32(1.0))).astype(np.float64)
        dt = np.abs(tr - t32.astype(np.float64))
        if not (dt <= tol).all():
            bad.append("|t - t_ref| = %s (bar %s)" % (dt, tol))
    else:
        s64, t64 = s.astype(np.float64), t.astype(np.float64)
        err = np.abs(s64 @ R.T + tr - t64).max()
        bar = 1e-5 * (1.0 + max(np.abs(s64).max(), np.abs(t64).max()))
        if not err <= bar:
            bad.append("|T s - t| = %.3g (bar %.3g)" % (err, bar))
    return bad


# ---- clouds (float32, n x 3), every one returns (source, target) with source[i] <-> target[i] -----
def generic(rng, n=300, max_angle=0.5, centre=(0.0, 0.0, 0.0), max_shift=1.0):
    tgt = (np.asarray(centre) + rng.uniform(-10, 10, (n, 3))).astype(F32)
    return move(tgt, random_rot(rng, max_angle), rng.uniform(-max_shift, max_shift, 3)), tgt


def plane_points(rng, n, normal=None):
    """n points within +-10 m on a random tilted plane through a random point."""
    nrm = rng.normal(size=3) if normal is None else np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    e0 = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
    e0 /= np.linalg.norm(e0)
    e1 = np.cross(nrm, e0)
    uv = rng.uniform(-7, 7, (n, 2))
    return (rng.uniform(-2, 2, 3) + uv[:, :1] * e0 + uv[:, 1:] * e1).astype(F32)


def tilted_plane(rng, n=300, moved=False):
    tgt = plane_points(rng, n)
    if not moved:
        return tgt.copy(), tgt
    return move(tgt, random_rot(rng, 0.05), rng.uniform(-0.2, 0.2, 3)), tgt


def axis_plane(rng, n=300, exact=True):
    """z = const; the source is an in-plane motion, so its z is the same constant.  `exact`: the
    constant is a power of two (or 0), for which the uncentred sums give sigma an exact zero row
    and column."""
    c = F32(rng.choice([0.0, 0.5, -1.0, 2.0, -4.0])) if exact else F32(rng.uniform(-3, 3))
    tgt = rng.uniform(-10, 10, (n, 3)).astype(F32)
    tgt[:, 2] = c
    src = move(tgt, rot([0, 0, 1], rng.uniform(-0.05, 0.05)), np.append(rng.uniform(-0.2, 0.2, 2), 0.0))
    src[:, 2] = c
    return src, tgt


def mirrored_slab(rng, n=300):
    """A slab 1 m thick mirrored through its mid-plane (then moved a little): sigma has full rank
    and a negative determinant, and the best proper rotation needs the -1."""
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    flat = plane_points(rng, n, nrm).astype(np.float64)
    h = rng.uniform(-0.5, 0.5, (n, 1))
    tgt = (flat + h * nrm).astype(F32)
    src = move(flat - h * nrm, random_rot(rng, 0.02), rng.uniform(-0.1, 0.1, 3))
    return src, tgt


def line(rng, n=300, axis_aligned=False):
    if axis_aligned:  # exactly rank 1 in float: x varies, y and z are powers of two
        tgt = np.zeros((n, 3), F32)
        tgt[:, 0], tgt[:, 1], tgt[:, 2] = rng.uniform(-10, 10, n), 2.0, -0.5
        src = tgt.copy()
        src[:, 0] += F32(0.25)
        return src, tgt
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    tgt = (rng.uniform(-2, 2, 3) + rng.uniform(-10, 10, (n, 1)) * d).astype(F32)
    return move(tgt, random_rot(rng, 0.05), rng.uniform(-0.2, 0.2, 3)), tgt
