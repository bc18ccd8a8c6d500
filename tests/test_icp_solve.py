"""The ICP's transformation estimate (csrc/fbr_icp_solve.h: the 3x3 Jacobi SVD and the Umeyama step
k_icp_solve calls) compiled for the CPU through tests/native/host_probe.cpp and compared with a
centred float64 Umeyama, on the inputs the loop-closure fixture never reaches: planar, collinear
and coincident correspondences, a mirrored slab (a legitimate -1), a cloud far from the origin.

Bars: tests/icp_cases.py.  The planar cases fail with S = diag(1, 1, sign det(sigma)): det(sigma) is
rounding noise there, and a negative one turns R into a reflection.
"""
import ctypes

import numpy as np
import pytest

import icp_cases as C
import loop_model as M

DRAWS = 300


def solve(probe_lib, sums):
    sums = np.ascontiguousarray(np.asarray(sums, np.float64).reshape(-1, 17))
    T = np.zeros((len(sums), 12), np.float32)
    probe_lib.probe_icp_umeyama.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    probe_lib.probe_icp_umeyama.restype = None
    probe_lib.probe_icp_umeyama(sums.ctypes.data, T.ctypes.data, len(sums))
    return T.reshape(-1, 3, 4)


CASES = {
    # name: (seed, cloud maker, rotation unique)
    "generic": (11, lambda rng: C.generic(rng), True),
    "plane_identical": (12, lambda rng: C.tilted_plane(rng, moved=False), True),
    "plane_moved": (13, lambda rng: C.tilted_plane(rng, moved=True), True),
    "axis_plane_exact": (14, lambda rng: C.axis_plane(rng, exact=True), True),
    "axis_plane": (15, lambda rng: C.axis_plane(rng, exact=False), True),
    "mirrored_slab": (16, lambda rng: C.mirrored_slab(rng), True),
    "line": (17, lambda rng: C.line(rng), False),
    "line_axis_aligned": (18, lambda rng: C.line(rng, axis_aligned=True), False),
    "far_from_origin": (19, lambda rng: C.generic(rng, max_angle=0.05, centre=(2000.0, -1500.0, 30.0), max_shift=0.3), True),
}


def draws(name, n=DRAWS):
    seed, make, unique = CASES[name]
    rng = np.random.default_rng(seed)
    return [make(rng) for _ in range(n)], unique


def failures(solver, name, n=DRAWS):
    """[(draw, [failed bars])] of `solver` (sums -> T) over the case's draws."""
    clouds, unique = draws(name, n)
    T = solver(np.stack([C.sums17(s, t) for s, t in clouds]))
    out = []
    for k, (s, t) in enumerate(clouds):
        bad = C.check(T[k], s, t, unique)
        if bad:
            out.append((k, bad))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_solve_matches_centred_float64_umeyama(probe_lib, name):
    bad = failures(lambda sums: solve(probe_lib, sums), name)
    print("%s: %d of %d draws fail" % (name, len(bad), DRAWS))
    assert not bad, (len(bad), bad[:3])


def test_case_inputs_are_what_they_claim():
    """Conditions on the inputs: sigma of the exact axis-aligned plane has a zero row and column from
    the uncentred sums; the mirrored slab has det(sigma) < 0 at full rank; the planes have w2 ~ 0."""
    for s, t in draws("axis_plane_exact", 20)[0]:
        v = C.sums17(s, t)
        sig = v[7:16].reshape(3, 3) / v[0] - np.outer(v[4:7] / v[0], v[1:4] / v[0])
        assert (sig[2] == 0).all() and (sig[:, 2] == 0).all() and np.linalg.matrix_rank(sig) == 2
    for s, t in draws("mirrored_slab", 20)[0]:
        s64, t64 = s.astype(np.float64), t.astype(np.float64)
        sig = (t64 - t64.mean(0)).T @ (s64 - s64.mean(0)) / len(s)
        w = np.linalg.svd(sig, compute_uv=False)
        assert np.linalg.det(sig) < 0 and w[2] > 1e-4 * w[0]
    for name in ("plane_identical", "plane_moved"):
        for s, t in draws(name, 20)[0]:
            assert C.reference(s, t)[2][2] < 1e-10


def test_mirrored_slab_keeps_its_minus_one(probe_lib):
    """The legitimate -1: R is the proper rotation next to the mirror (close to the identity here),
    not U V^T, which would be the reflection itself."""
    for s, t in draws("mirrored_slab", 20)[0]:
        T = solve(probe_lib, C.sums17(s, t))[0]
        assert np.linalg.det(T[:, :3].astype(np.float64)) > 0.999
        assert np.abs(T[:, :3] - np.eye(3)).max() < 0.05


def test_coincident_source_points(probe_lib):
    """sigma = 0.  Exactly (sums of a power-of-two count of one source and one target point): R = I
    and t = mt - ms.  With distinct targets sigma is rounding noise: any proper rotation, and the
    source point lands on the targets' mean."""
    rng = np.random.default_rng(21)
    for _ in range(DRAWS):
        p, q = rng.uniform(-10, 10, 3).astype(np.float32), rng.uniform(-10, 10, 3).astype(np.float32)
        n = 256
        p64, q64 = p.astype(np.float64), q.astype(np.float64)
        sums = np.concatenate([[n], n * p64, n * q64, (n * np.outer(q64, p64)).ravel(), [0.0]])
        T = solve(probe_lib, sums)[0]
        assert np.array_equal(T[:, :3], np.eye(3, dtype=np.float32))
        assert np.array_equal(T[:, 3], (q64 - p64).astype(np.float32))
        assert not C.check(T, np.tile(p, (n, 1)), np.tile(q, (n, 1)), unique=False)

        tgt = rng.uniform(-10, 10, (300, 3)).astype(np.float32)
        src = np.tile(p, (300, 1))
        T = solve(probe_lib, C.sums17(src, tgt))[0]
        mean = np.tile(tgt.astype(np.float64).mean(0).astype(np.float32), (300, 1))
        assert not C.check(T, src, mean, unique=False)


def test_model_umeyama_is_a_rotation_on_planes():
    """tests/loop_model.py's umeyama (the reference of the GPU tests) under the same bars."""
    for name in ("plane_identical", "plane_moved", "mirrored_slab", "generic"):
        clouds, unique = draws(name, 100)
        for s, t in clouds:
            assert not C.check(M.umeyama(s, t), s, t, unique)
