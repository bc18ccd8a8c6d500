"""The cases of the per-query Gauss-Newton tests (tests/test_gn_model.py on the CPU,
tests/test_gn_rows.py on the device): five neighbours, a map-frame query, a scan-frame point and the
trig of a pose per case, built where the fits, the gates and the residuals go wrong.  NumPy only,
fixed seeds.  `well` marks the cases a float64 reference can judge (well conditioned, not built on a
degenerate fit); every case, marked or not, is compared with the device bit for bit.
"""
import numpy as np

import gn_model as G
from knn_model import _nudge

F = np.float32
CORNER, SURF = 0, 1
# roll, pitch, yaw, x, y, z: zero, small and +-pi/2 pitch (float32's nearest), general angles
POSES = [(0, 0, 0, 0, 0, 0), (0.01, -0.02, 0.03, 1, 2, 3), (0.3, 1e-4, -2.0, -4, 5, 0.5), (-0.7, np.pi / 2, 1.1, 0, 0, 0),
         (2.5, -np.pi / 2, -0.4, 10, -20, 1), (-3.0, 0.9, 3.1, 0.1, 0.2, 0.3), (0.0, 1e-8, 0.0, 0, 0, 0),
         (1.0, -1.2, 0.5, 100, 50, -2)]


class _Set:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def add(self, kind, tag, nbr, q, well=True):
        n = len(self.rows)
        p = self.rng.uniform(-20, 20, 3)
        self.rows.append(dict(kind=kind, tag=tag, nbr=np.asarray(nbr, F).reshape(5, 3), q=np.asarray(q, F).reshape(3),
                              p=p.astype(F), pose=np.asarray(POSES[n % len(POSES)], F), well=bool(well)))


def _basis(rng):
    m = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return m * np.sign(np.linalg.det(m))


def _line_cluster(rng, centre, perp, along=0.4, R=None):
    """Five points: spread `along` on the first axis of a random basis, `perp` on the other two."""
    R = _basis(rng) if R is None else R
    t = rng.standard_normal((5, 3)) * (along, perp, perp * 0.6)
    return np.asarray(centre) + t @ R.T


def _plane_cluster(rng, centre, noise, R=None):
    R = _basis(rng) if R is None else R
    t = np.concatenate([rng.uniform(-0.6, 0.6, (5, 2)), rng.standard_normal((5, 1)) * noise], axis=1)
    return np.asarray(centre) + t @ R.T


def build():
    s = _Set(20240921)
    rng = s.rng
    centre = lambda far=0.0: rng.uniform(-8, 8, 3) + far * np.array([0.6, -0.8, 0.02])  # noqa: E731

    # ---- corner_fit: clusters along a line, the eigenvalue ratio swept across 3 from both sides ----
    for perp in np.geomspace(0.02, 0.5, 40):
        c = centre()
        nb = _line_cluster(rng, c, perp)
        s.add(CORNER, "line_sweep", nb, c + rng.standard_normal(3) * 0.15)
    for n in range(16):  # fat clusters: no line
        c = centre()
        s.add(CORNER, "line_fat", _line_cluster(rng, c, rng.uniform(0.3, 0.6)), c + rng.standard_normal(3) * 0.15)
    for n in range(24):  # thin clusters, queries at 0.05 .. 0.6 m
        c = centre()
        nb = _line_cluster(rng, c, 0.01)
        s.add(CORNER, "line_thin", nb, c + rng.standard_normal(3) * rng.uniform(0.05, 0.4))
    # D1[0] == 3 * D1[1] exactly: x = (15, -15, 0, 0, 0) u, y = (5, 5, -10, 0, 0) u, z constant:
    # covariance diag(90, 30, 0) u^2 with every sum exact and no rotation in the Jacobi; rejected
    # (the gate is >).  Its neighbours on either side: x scaled by 16 / 15 and by 14 / 15.
    u = 2.0 ** -6
    for tag, sx in (("ratio_exact_3", 15.0), ("ratio_above_3", 16.0), ("ratio_below_3", 14.0)):
        nb = np.array([(sx * u, 5 * u, 0.5), (-sx * u, 5 * u, 0.5), (0, -10 * u, 0.5), (0, 0, 0.5), (0, 0, 0.5)])
        s.add(CORNER, tag, nb, (0.03125, 0.0625, 0.625), well=tag != "ratio_exact_3")
    for ax in range(3):  # axis-aligned lines: exactly collinear, no rotation
        nb = np.zeros((5, 3))
        nb[:, ax] = (-0.5, -0.25, 0.0, 0.25, 0.5)
        nb += (1.0, -2.0, 0.5)
        q = np.array((1.0, -2.0, 0.5))
        q[(ax + 1) % 3] += 0.25
        s.add(CORNER, "axis_line", nb, q)
        s.add(CORNER, "query_on_line", nb, (1.0, -2.0, 0.5), well=False)  # a012 = 0: NaN coefficients, s = 1
        nb2 = nb.copy()  # diagonal covariance with spread on the other axes
        nb2[:, (ax + 1) % 3] += (0.0625, -0.0625, 0.0, 0.0625, -0.0625)
        s.add(CORNER, "axis_line_diag", nb2, q)
    R = _basis(rng)
    nb = np.outer((-0.5, -0.2, 0.0, 0.3, 0.4), R[:, 0]) + (2.0, 3.0, -1.0)
    s.add(CORNER, "collinear", nb, (2.1, 3.2, -0.9))
    s.add(CORNER, "identical", np.tile((1.5, -2.5, 0.75), (5, 1)), (1.5, -2.4, 0.75), well=False)
    nb = np.array([(0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0)]) + (3.0, 1.0, 2.0)
    s.add(CORNER, "two_equal_largest", nb, (3.0, 1.0, 2.2))
    for far in (500.0, 5000.0):  # cancellation in the centred sums
        for n in range(8):
            c = centre(far)
            nb = _line_cluster(rng, c, (0.01, 0.3)[n % 2])
            s.add(CORNER, "far_%d" % far, nb, c + rng.standard_normal(3) * 0.1, well=False)
    # ---- corner_apply: s across 0.1 (distance to the line across 1 m), far queries ----
    nb = np.zeros((5, 3))
    nb[:, 0] = (-0.5, -0.25, 0.0, 0.25, 0.5)
    for n in (-32, -3, -2, -1, 0, 1, 2, 3, 32):
        s.add(CORNER, "s_at_0.1", nb, (0.0, float(_nudge(1.0, n)), 0.0), well=abs(n) > 3)
    for d in (0.5, 0.99, 1.01, 1.5, 5.0, 60.0):
        s.add(CORNER, "query_far", nb, (0.125, d * 0.6, d * 0.8))

    # ---- surf_fit ----
    for noise in np.geomspace(0.002, 0.4, 40):
        c = centre()
        nb = _plane_cluster(rng, c, noise)
        s.add(SURF, "plane_sweep", nb, c + rng.standard_normal(3) * 0.3)
    for n in range(24):
        c = centre()
        nb = _plane_cluster(rng, c, 0.005)
        s.add(SURF, "plane_thin", nb, c + rng.standard_normal(3) * rng.uniform(0.05, 0.5))
    sq = np.array([(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 0, 0)]) * 0.5
    s.add(SURF, "coplanar", sq + (0.25, -0.5, 1.0), (0.5, 0.25, 1.125))
    s.add(SURF, "coplanar", sq[:, [2, 0, 1]] + (2.0, 0.25, -0.5), (2.25, 0.5, 0.0))
    # one neighbour 0.2 m from the fitted plane: four corners at z = z0, the centre at z0 + h; the
    # least-squares plane is z = sum z^2 / sum z, and the centre's distance to it, 8 |h| / (10 + h)
    # for z0 = 2, reaches 0.2 at h = 2 / 7.8 and at h = -2 / 8.2; h nudged around both
    for h in (2.0 / 7.8, -2.0 / 8.2):
        for n in (-64, -8, -3, -2, -1, 0, 1, 2, 3, 8, 64):
            nb = sq + (0.0, 0.0, 2.0)
            nb[4, 2] = float(_nudge(2.0 + h, n))
            s.add(SURF, "plane_gate_0.2", nb, (0.125, 0.25, 2.0625), well=abs(n) > 8)
    nb = np.outer((-0.5, -0.2, 0.0, 0.3, 0.4), R[:, 1]) + (2.0, 3.0, -1.0)
    s.add(SURF, "collinear", nb, (2.1, 3.1, -1.0), well=False)  # rank-deficient column-pivoted solve
    # a plane through the origin: a x + b y + c z = -1 has no solution; the pinned solver's answer stands
    s.add(SURF, "through_origin", sq, (0.25, 0.125, 0.03125), well=False)
    nb = rng.uniform(-1, 1, (5, 3))
    nb[:, 2] = -(nb[:, 0] + nb[:, 1])  # x + y + z = 0 up to rounding
    s.add(SURF, "through_origin", nb, (0.5, -0.25, -0.2), well=False)
    s.add(SURF, "identical", np.tile((1.0, 2.0, 3.0), (5, 1)), (1.0, 2.0, 3.1), well=False)
    for far in (500.0, 5000.0):
        for n in range(8):
            c = centre(far)
            nb = _plane_cluster(rng, c, (0.005, 0.15)[n % 2])
            s.add(SURF, "far_%d" % far, nb, c + rng.standard_normal(3) * 0.1, well=False)
    # ---- surf_apply: the query at the origin (sqrt(sqrt(0))), s across 0.1, far queries ----
    pl = sq + (0.0, 0.0, 1.0)  # the plane z = 1
    s.add(SURF, "query_origin", pl, (0.0, 0.0, 0.0), well=False)
    # on the z axis |1 - z| / sqrt(z) = 1 at z = (3 + sqrt(5)) / 2: s = 0.1 there
    zc = (3.0 + np.sqrt(5.0)) / 2.0
    for n in (-64, -6, -3, -2, -1, 0, 1, 2, 3, 6, 64):
        s.add(SURF, "s_at_0.1", pl, (0.0, 0.0, float(_nudge(zc, n))), well=abs(n) > 6)
    for q in ((0.25, 0.25, 1.01), (0.1, 0.2, 1.6), (50.0, 50.0, 50.0), (0.0, 3.0, -4.0), (1e-3, 0.0, 1.0)):
        s.add(SURF, "query_far", pl, q)
    return pack(s.rows)


def pack(rows):
    n = len(rows)
    c = dict(kind=np.array([r["kind"] for r in rows], np.int32), tag=[r["tag"] for r in rows],
             nbr=np.stack([r["nbr"] for r in rows]), q=np.stack([r["q"] for r in rows]), p=np.stack([r["p"] for r in rows]),
             pose=np.stack([r["pose"] for r in rows]), well=np.array([r["well"] for r in rows], bool))
    c["trig"] = np.stack([G.trig_of(pose) for pose in c["pose"]])
    assert c["nbr"].shape == (n, 5, 3) and c["trig"].shape == (n, 6)
    return c


def device_input(c):
    """(n, 28) float32 rows of fbr_selftest_gn_rows."""
    n = len(c["kind"])
    return np.concatenate([c["kind"].astype(F).reshape(n, 1), c["nbr"].reshape(n, 15), c["q"], c["p"], c["trig"]], axis=1)


def model_rows(c):
    """The model's outputs in fbr_selftest_gn_rows's conventions: what a rejected stage would have
    written is 0."""
    n = len(c["kind"])
    out = dict(fit_ok=np.zeros(n, bool), fit=np.zeros((n, 6), F), ok=np.zeros(n, bool), coeff=np.zeros((n, 4), F),
               row=np.zeros((n, 6), F), b=np.zeros(n, F))
    for i in range(n):
        corner = c["kind"][i] == CORNER
        fok, f = (G.corner_fit if corner else G.surf_fit)(c["nbr"][i])
        out["fit_ok"][i] = fok
        if not fok:
            continue
        out["fit"][i, :len(f)] = f
        ok, coeff = (G.corner_apply if corner else G.surf_apply)(f, c["q"][i])
        out["ok"][i], out["coeff"][i] = ok, coeff
        if ok:
            out["row"][i], out["b"][i] = G.row(c["trig"][i], c["p"][i], coeff)
    return out
