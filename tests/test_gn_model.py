"""tests/gn_model.py, the float32 restatement the device is held to bit for bit, against a float64
reference that shares no code with it: np.linalg.eigh for the line, np.linalg.lstsq for the plane,
vector formulas for the point-to-line and point-to-plane distance and direction, and central
differences of coeff . (T(pose) p) for the LMOptimization row.  No GPU.

Measured on the cases of tests/gn_cases.py that a float64 reference can judge (`well`, clear of the
gates by 1e-3 relative, and for the residuals a fit both sides accept): the model's largest deviation
from float64, and the bound, set to twice that:

    line points c +- 0.1 v, absolute                          measured 9.24e-07   bound 1.85e-06
    plane (pa, pb, pc, pd), absolute                           measured 2.39e-05   bound 4.8e-05
    coefficients, relative to max(1, |coeff|)                  measured 4.10e-05   bound 8.2e-05
    row, relative to (|p|_1 + 1) max(1, |coeff|)               measured 2.74e-05   bound 5.5e-05
    row . delta vs central difference, rel. to |row| |delta|   measured 5.31e-07   bound 1.07e-06

(The plane of a cluster up to 14 m from the origin comes from a float32 solve of a x + b y + c z = -1,
and the coefficients carry the fit's error times the query's distance from the fitted points.)  The
bounds constrain the model alone: the device tests demand equality with it.
"""
import numpy as np

import gn_cases as C
import gn_model as G
import knn_model as K

F = np.float32
BOUND_LINE, BOUND_PLANE, BOUND_COEFF, BOUND_ROW, BOUND_CDIFF = 1.85e-06, 4.8e-05, 8.2e-05, 5.5e-05, 1.07e-06
GATE_CLEAR = 1e-3


# ------------------------------------------------------------------------------------ float64 reference
def ref_corner(nbr, q):
    """-> dict(ratio, fit_ok, pts (2, 3), dist, s, coeff) in float64."""
    nbr, q = np.asarray(nbr, np.float64), np.asarray(q, np.float64)
    c = nbr.mean(0)
    w, v = np.linalg.eigh((nbr - c).T @ (nbr - c) / 5.0)
    lam0, lam1, axis = w[2], w[1], v[:, 2]
    d = q - c
    perp = d - (d @ axis) * axis
    dist = np.linalg.norm(perp)
    s = 1.0 - 0.9 * dist
    return dict(ratio=lam0 / lam1 if lam1 > 0 else np.inf, fit_ok=lam0 > 3.0 * lam1, pts=np.stack([c + 0.1 * axis, c - 0.1 * axis]),
                gate=dist, s=s, ok=s > 0.1, coeff=np.concatenate([s * perp / dist, [s * dist]]) if dist > 0 else np.full(4, np.nan))


def ref_surf(nbr, q):
    nbr, q = np.asarray(nbr, np.float64), np.asarray(q, np.float64)
    x = np.linalg.lstsq(nbr, -np.ones(5), rcond=None)[0]
    nrm = np.linalg.norm(x)
    n, pd = x / nrm, 1.0 / nrm
    far = np.abs(nbr @ n + pd).max()
    pd2 = q @ n + pd
    s = 1.0 - 0.9 * abs(pd2) / np.sqrt(np.linalg.norm(q))
    return dict(gate=far, fit_ok=far <= 0.2, plane=np.concatenate([n, [pd]]), s=s, ok=s > 0.1,
                coeff=np.concatenate([s * n, [s * pd2]]))


def clear(value, gate):
    return abs(value - gate) > GATE_CLEAR * gate


def test_case_table_meets_its_conditions():
    """At least a third of each kind accepted and a fifth rejected by the model alone; the designed
    gate cases land on both sides; the exact-ratio case is exact."""
    c = C.build()
    m = C.model_rows(c)
    assert len(c["kind"]) >= 200
    for kind in (C.CORNER, C.SURF):
        k = c["kind"] == kind
        acc = m["ok"][k].mean()
        print("kind %d: %d cases, accepted %.3f, rejected %.3f" % (kind, k.sum(), acc, 1 - acc))
        assert acc >= 1 / 3 and 1 - acc >= 1 / 5, (kind, acc)
    tags = np.array(c["tag"])
    for kind, tag, field in ((C.SURF, "plane_gate_0.2", "fit_ok"), (C.CORNER, "s_at_0.1", "ok"), (C.SURF, "s_at_0.1", "ok"),
                             (C.CORNER, "line_sweep", "fit_ok"), (C.SURF, "plane_sweep", "fit_ok")):
        got = m[field][(tags == tag) & (c["kind"] == kind)]
        assert got.any() and not got.all(), (kind, tag)
    # D1[0] == 3 * D1[1] exactly, and rejected: the gate is a strict >
    i = c["tag"].index("ratio_exact_3")
    nn = c["nbr"][i].astype(np.float64)
    cov = np.cov(nn.T, bias=True)
    assert np.array_equal(cov, np.diag(np.diag(cov))) and cov[0, 0] == 3 * cov[1, 1] and F(cov[0, 0]) == cov[0, 0]
    assert not m["fit_ok"][i] and m["fit_ok"][c["tag"].index("ratio_above_3")] and not m["fit_ok"][c["tag"].index("ratio_below_3")]
    # the undefined cases are what they were built to be
    on = [i for i, t in enumerate(c["tag"]) if t == "query_on_line"]
    assert all(m["ok"][i] and np.isnan(m["coeff"][i, :3]).all() and m["coeff"][i, 3] == 0 for i in on)
    assert not m["ok"][c["tag"].index("query_origin")] and m["fit_ok"][c["tag"].index("query_origin")]
    assert not m["fit_ok"][c["tag"].index("identical")]  # the corner one: covariance 0


def test_model_agrees_with_float64_reference():
    c = C.build()
    m = C.model_rows(c)
    dev = dict(line=(0.0, -1), plane=(0.0, -1), coeff=(0.0, -1), row=(0.0, -1))
    n_fit = n_res = 0

    def note(what, d, i):
        if d > dev[what][0]:
            dev[what] = (d, i)

    for i in np.flatnonzero(c["well"]):
        corner = c["kind"][i] == C.CORNER
        r = (ref_corner if corner else ref_surf)(c["nbr"][i], c["q"][i])
        # ---- gates: clear of 3 / 0.2 -> the same decision ----
        if corner:
            if not clear(r["ratio"], 3.0):
                continue
        elif not clear(r["gate"], 0.2):
            continue
        assert bool(m["fit_ok"][i]) == bool(r["fit_ok"]), (i, c["tag"][i])
        n_fit += 1
        if not r["fit_ok"]:
            continue
        if corner:
            pts = m["fit"][i].astype(np.float64).reshape(2, 3)
            d = min(np.abs(pts - r["pts"]).max(), np.abs(pts[::-1] - r["pts"]).max())  # the axis' sign is free
            note("line", d, i)
        else:
            d = np.abs(m["fit"][i, :4].astype(np.float64) - r["plane"]).max()
            note("plane", d, i)
        if not clear(r["s"], 0.1):
            continue
        assert bool(m["ok"][i]) == bool(r["ok"]), (i, c["tag"][i], r["s"])
        n_res += 1
        scale = max(1.0, np.abs(r["coeff"]).max())  # a far query's s d grows with d^2
        note("coeff", np.abs(m["coeff"][i].astype(np.float64) - r["coeff"]).max() / scale, i)
        if not r["ok"]:
            continue
        # ---- the row against the analytic Jacobian in float64 (row_ref below) of the reference's coeff ----
        p = c["p"][i].astype(np.float64)
        want = row_ref(c["pose"][i].astype(np.float64), p, r["coeff"][:3])
        note("row", np.abs(m["row"][i].astype(np.float64) - want).max() / ((np.abs(p).sum() + 1.0) * scale), i)
        assert m["b"][i] == -m["coeff"][i, 3]
    print("largest deviations from float64:", {k: "%.2e (%s)" % (v[0], c["tag"][v[1]]) for k, v in dev.items()},
          "fits", n_fit, "residuals", n_res)
    for what, bound in (("line", BOUND_LINE), ("plane", BOUND_PLANE), ("coeff", BOUND_COEFF), ("row", BOUND_ROW)):
        assert dev[what][0] <= bound, (what, dev[what], c["tag"][dev[what][1]])
    assert n_fit >= 120 and n_res >= 100


def transform64(pose, p):
    T = K.pose_matrix64(pose)
    return T[:, :3] @ p + T[:, 3]


def row_ref(pose, p, n, h=1e-5):
    """d/dpose of n . (T(pose) p) by central differences in float64 (6,)."""
    out = np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        out[k] = (n @ transform64(pose + e, p) - n @ transform64(pose - e, p)) / (2 * h)
    return out


def test_row_is_the_derivative_it_claims_to_be():
    """row . delta against a central difference of coeff.xyz . (T(pose + delta) p) in float64, for
    random poses (pitch inside +-1.5), points, directions and steps."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(400):
        pose = np.concatenate([rng.uniform(-3.1, 3.1, 1), rng.uniform(-1.5, 1.5, 1), rng.uniform(-3.1, 3.1, 1),
                               rng.uniform(-50, 50, 3)]).astype(F)
        p = rng.uniform(-30, 30, 3).astype(F)
        n = rng.standard_normal(3)
        coeff = np.concatenate([n / np.linalg.norm(n) * rng.uniform(0.2, 1.0), [rng.uniform(-0.5, 0.5)]]).astype(F)
        r, b = G.row(G.trig_of(pose), p, coeff)
        assert b == -coeff[3]
        delta = rng.standard_normal(6) * 1e-5
        p64, n64, pose64 = p.astype(np.float64), coeff[:3].astype(np.float64), pose.astype(np.float64)
        cd = (n64 @ transform64(pose64 + delta, p64) - n64 @ transform64(pose64 - delta, p64)) / 2.0
        got = r.astype(np.float64) @ delta
        rel = abs(got - cd) / (np.linalg.norm(r.astype(np.float64)) * np.linalg.norm(delta))
        worst = max(worst, rel)
    print("row . delta vs central difference, largest relative deviation: %.2e" % worst)
    assert worst <= BOUND_CDIFF


def test_item_partial_and_solve_step():
    """The partial is the exact sum rounded once; the step solves the normal equations it is given."""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((256, 6)).astype(F) * F(7.0)
    b = rng.standard_normal(256).astype(F)
    ok = rng.random(256) < 0.7
    part = G.item_partial(rows, b, ok)
    assert part[27] == int(ok.sum()) and len(part) == 28
    from fractions import Fraction
    k = 7  # AtA[1][2]
    exact = sum(Fraction(float(rows[i, 1])) * Fraction(float(rows[i, 2])) for i in range(256) if ok[i])
    assert part[k] == float(exact)
    assert part[21] == float(sum(Fraction(float(rows[i, 0])) * Fraction(float(b[i])) for i in range(256) if ok[i]))
    pose = np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0], F)
    new, X = G.solve_step(part, pose)
    A = (rows[ok].astype(np.float64).T @ rows[ok].astype(np.float64))
    want = np.linalg.solve(A, rows[ok].astype(np.float64).T @ b[ok].astype(np.float64))
    assert np.allclose(X, want, rtol=1e-4, atol=1e-6) and np.array_equal(new, pose + X) and new.dtype == F
    sing = np.zeros(28)  # diag(1, 1, 1, 1, 1, 1e-8): |R[5][5]| below cv::solve's eps, X = 0
    sing[[0, 6, 11, 15, 18, 20]] = (1, 1, 1, 1, 1, 1e-8)
    sing[21:27] = 1.0
    new, X = G.solve_step(sing, pose)
    assert not X.any() and np.array_equal(new, pose)
    dR, dT = G.step_deltas(np.array([1e-4, 0, 0, 0, 3e-4, 4e-4], F))
    assert abs(dR - 57.29578e-4) < 1e-8 and abs(dT - 0.05) < 1e-7
