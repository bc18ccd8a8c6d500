"""Registration information on the CPU: csrc/fbr_reg_info.h, built for the host by
tests/native/info_probe.cpp, against tests/info_model.py.  No GPU is needed.

  * the header's Jacobi against numpy.linalg.eigh on the model's H of the GPU tests' worlds and on
    designed matrices (rank 0, 3, 5, repeated eigenvalues, H scaled by 1e+-8);
  * the chart map S against central differences of the chart (R Exp(w), t + R v) in float64 at the
    eight poses of gn_cases.POSES (at pitch = +-pi/2: finite, and equal to the model);
  * the covariance assembly, the flagged records and fbr_reg_info_variances' floors.

The Jacobi tolerance is the backward-error bound k 6 2^-52 ||H||_F with k = 15 x the header's sweep
limit (one unit per rotation; 15 rotations per sweep, 16 sweeps at most: k = 240), taken from the
routine's structure and not from its results.  Eigenvalues of a symmetric matrix move by at most the
2-norm of a perturbation (Weyl), so the bound holds for each eigenvalue.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import gn_cases
import info_cases as C
import info_model as M
import knn_model as K
from feature_base_pointcloud_registration_amd import api, build
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_INFO_BAD_POSE, FBR_INFO_FEW_ROWS, FBR_INFO_NO_ROWS,
                                                                FBR_INFO_NOT_REGISTERED, REG_INFO, FbrInfoParams, info_params)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def jacobi_tol(H):
    return M.jacobi_k(M.probe().probe_info_sweep_limit()) * 6 * M.EPS * np.linalg.norm(H)


@pytest.fixture(scope="module")
def world_H():
    """name -> (record, rows, mag) of the model on the GPU tests' worlds."""
    out = {}
    t = C.tiny()
    mc, ms = K.xyz_of(t["corner_map"]), K.xyz_of(t["surf_map"])
    for name, pose in (("tiny_gt", t["gt"]), ("tiny_guess", np.zeros(6, F))):
        out[name] = M.info(mc, ms, K.xyz_of(t["corner"]), K.xyz_of(t["surf"]), pose, K.CROP_HALF)
    for name, kw in (("corridor_0", {}), ("corridor_90", dict(yaw=np.pi / 2)), ("corridor_end", dict(end_wall=True))):
        c = C.corridor(**kw)
        out[name] = M.info(K.xyz_of(c["corner_map"]), K.xyz_of(c["surf_map"]), K.xyz_of(c["corner"]), K.xyz_of(c["surf"]),
                           c["pose"], C.CORRIDOR_CROP)
    return out


def designed():
    rng = np.random.default_rng(7)
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    mk = lambda d: (Q * np.asarray(d, float)) @ Q.T  # noqa: E731
    sym = lambda A: (A + A.T) / 2  # noqa: E731
    base = sym(mk([3e2, 5e3, 7e3, 2e4, 9e4, 4e5]))
    return {"rank0": np.zeros((6, 6)), "rank3": sym(mk([0, 0, 0, 1e3, 2e3, 5e4])), "rank5": sym(mk([0, 4e2, 1e3, 2e3, 5e4, 9e4])),
            "repeated": sym(mk([1e3, 1e3, 1e3, 7e4, 7e4, 2e5])), "identity": np.eye(6) * 250.0, "diagonal": np.diag([6.0, 5, 4, 3, 2, 1]),
            "scaled_up": base * 1e8, "scaled_down": base * 1e-8, "general": base}


def check_jacobi(name, H):
    eig, vec, sweeps = M.probe_jacobi(H)
    want = np.linalg.eigvalsh(H)
    tol = jacobi_tol(H)
    err = np.abs(eig - want).max()
    print("%s: %d sweeps, |eig - eigh| %.3g, bound %.3g" % (name, sweeps, err, tol))
    assert sweeps < M.probe().probe_info_sweep_limit(), name  # it converged: the limit did not end it
    assert (np.diff(eig) >= 0).all(), (name, eig)
    assert err <= tol, (name, err, tol)
    # rows are orthonormal eigenvectors: V V^T = I and V^T diag(eig) V = H, within the same backward error
    assert np.abs(vec @ vec.T - np.eye(6)).max() <= M.jacobi_k(16) * 6 * M.EPS, name
    assert np.linalg.norm(vec.T @ np.diag(eig) @ vec - H) <= max(tol, 1e-300), (name, np.linalg.norm(vec.T @ np.diag(eig) @ vec - H), tol)


@pytest.mark.parametrize("name", list(designed()))
def test_jacobi_on_designed_matrices(name):
    check_jacobi(name, designed()[name])


def test_jacobi_on_the_worlds(world_H):
    for name, (rec, _, _) in world_H.items():
        assert rec["flags"] == 0 and rec["n_rows"].sum() > 100, (name, rec["flags"], rec["n_rows"])
        check_jacobi(name, rec["H"])
    # what the GPU tests rely on: the corridor does not observe x, its end wall does
    # (the tiny set's 360 rows sit just above the floor at the true pose and straddle it at the guess)
    for name, rank in (("tiny_gt", 6), ("tiny_guess", None), ("corridor_0", 5), ("corridor_90", 5), ("corridor_end", 6)):
        rec = world_H[name][0]
        print(name, "eig", rec["eig"], "var_tangent", rec["var_tangent"])
        assert rank is None or rec["rank"] == rank, (name, rec["eig"])
        assert np.abs(rec["eig"] - M.EIG_FLOOR).min() > 1.0, (name, rec["eig"])  # no eigenvalue at the floor: 1e9 x the Jacobi bound


# ------------------------------------------------------------------------------------ S
def _exp(w):
    t = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + math.sin(t) / t * W + (1 - math.cos(t)) / t ** 2 * W @ W


def _log(R):
    t = math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2)))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return v if t < 1e-9 else v * t / math.sin(t)


def _Rt(p):
    T = K.pose_matrix64(p)
    return T[:, :3], T[:, 3]


def chart_fd(pose, h=1e-6):
    """d [w; v] / d pose by central differences: [w; v] = Local((R, t), (R', t')) of the chart."""
    p0 = np.asarray(pose, F).astype(np.float64)
    R0, t0 = _Rt(p0)
    S = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        (Rp, tp), (Rm, tm) = _Rt(p0 + d), _Rt(p0 - d)
        S[:3, k] = (_log(R0.T @ Rp) - _log(R0.T @ Rm)) / (2 * h)
        S[3:, k] = (R0.T @ (tp - t0) - R0.T @ (tm - t0)) / (2 * h)
    return S


@pytest.mark.parametrize("n", range(len(gn_cases.POSES)))
def test_chart_map_against_central_differences(n):
    pose = np.asarray(gn_cases.POSES[n], F)
    S, Sm = M.probe_chart(pose), M.chart(pose)
    assert np.isfinite(S).all()
    assert np.abs(S - Sm).max() <= 4 * M.EPS, (pose, np.abs(S - Sm).max())  # libm's sin / cos on both sides, one product
    # Exp(w) retracts, so the chart is consistent: R Exp(S_rot d) = R(p + d) to first order, everywhere
    # (pitch = +-pi/2 is a singularity of the pose, not of S: E loses rank there, finitely)
    assert np.abs(S - chart_fd(pose)).max() <= 1e-8, (pose, np.abs(S - chart_fd(pose)).max())
    R, _ = _Rt(pose.astype(np.float64))
    d = np.array([1e-7, -2e-7, 1.5e-7])
    Rn, _ = _Rt(pose.astype(np.float64) + np.concatenate([d, np.zeros(3)]))
    assert np.abs(R @ _exp(S[:3, :3] @ d) - Rn).max() <= 1e-12


# ------------------------------------------------------------------------------------ records
FIELDS = ("H", "g", "rss", "sigma2", "eig", "cov", "cov_tangent", "var_tangent")


def compare(rec, want, tag, h_err=0.0, s2_rel=0.0):
    """A device / probe record against the model's, eigen-dependent fields within the propagated
    Jacobi bound (info_model.cov_bound).  h_err: a bound of ||H_rec - H_want||_F (the device sums in
    another order), which moves the spectrum like the Jacobi's own backward error; s2_rel: a bound of
    sigma2's relative error, which scales the observed part of cov."""
    assert rec["flags"] == want["flags"] and rec["rank"] == want["rank"], (tag, rec["flags"], rec["rank"], want["rank"])
    assert list(rec["n_rows"]) == list(want["n_rows"]) and list(rec["n_query"]) == list(want["n_query"]), tag
    tau = M.jacobi_k(16) * 6 * M.EPS * np.linalg.norm(want["H"]) + h_err
    assert np.abs(rec["eig"] - want["eig"]).max() <= tau, (tag, rec["eig"], want["eig"])
    if want["flags"]:
        for f in FIELDS + ("evec",):
            assert np.array_equal(np.asarray(rec[f]), np.asarray(want[f])), (tag, f)
        return
    cb, gap = M.cov_bound(want, tau)
    assert gap > tau, (tag, gap, tau)
    # ||S||_2 <= sqrt(2) at any pose (E's largest singular value), so S . S^T at most doubles
    cb = cb + s2_rel * np.linalg.norm(want["cov"])
    assert np.linalg.norm(rec["cov"] - want["cov"]) <= cb + 64 * M.EPS * np.linalg.norm(want["cov"]), (tag, "cov", cb)
    assert np.linalg.norm(rec["cov_tangent"] - want["cov_tangent"]) <= 2 * cb + 128 * M.EPS * np.linalg.norm(want["cov"]), (tag, "cov_tangent")
    assert np.array_equal(np.diag(rec["cov_tangent"]), rec["var_tangent"]), tag
    assert np.array_equal(rec["cov"], rec["cov"].T) and np.array_equal(rec["H"], rec["H"].T), tag


def test_records_of_the_worlds(world_H):
    for name, (want, r, _) in world_H.items():
        acc, _ = M.sums(r)
        pose = {"tiny_gt": C.tiny()["gt"], "tiny_guess": np.zeros(6, F)}.get(name)
        if pose is None:
            pose = C.corridor(yaw=np.pi / 2 if name == "corridor_90" else 0.0)["pose"]
        rec = M.probe_record(acc, want["n_rows"], want["n_query"], pose)
        assert np.array_equal(rec["H"], want["H"]) and np.array_equal(rec["g"], want["g"]) and rec["rss"] == want["rss"], name
        assert rec["sigma2"] == want["sigma2"], name
        compare(rec, want, name)
    # the corridor: x is the unobserved direction, in the map frame and in the body frame
    for name, axis in (("corridor_0", 0), ("corridor_90", 1)):
        want = world_H[name][0]
        v0 = want["evec"][0]
        assert abs(v0[3]) > 0.999 and np.abs(np.delete(v0, 3)).max() < 0.04, (name, v0)
        assert int(np.argmax(want["var_tangent"][3:])) == axis, (name, want["var_tangent"])
        assert want["var_tangent"][3 + axis] > 0.99 * M.UNOBSERVED


def test_sigma2_and_floor_parameters(world_H):
    want, r, _ = world_H["corridor_0"]
    acc, _ = M.sums(r)
    pose = C.corridor()["pose"]
    for kw in (dict(sigma2=0.01), dict(eig_floor=1e3), dict(unobserved=25.0), dict(eig_floor=1e9)):
        rec, w = M.probe_record(acc, want["n_rows"], want["n_query"], pose, **kw), M.record(acc, want["n_rows"], want["n_query"], pose, **kw)
        compare(rec, w, str(kw))
    assert M.record(acc, want["n_rows"], want["n_query"], pose, eig_floor=1e9)["rank"] == 0


def test_flagged_records():
    acc = np.arange(29, dtype=np.float64) + 1.0
    ok_pose = np.zeros(6, F)
    cases = [((0, 0), ok_pose, 0, FBR_INFO_NO_ROWS), ((2, 3), ok_pose, 0, FBR_INFO_FEW_ROWS),
             ((40, 50), np.array([0, np.nan, 0, 0, 0, 0], F), 0, FBR_INFO_BAD_POSE),
             ((40, 50), np.array([0, 0, 0, np.inf, 0, 0], F), 0, FBR_INFO_BAD_POSE),
             ((40, 50), ok_pose, FBR_INFO_NOT_REGISTERED, FBR_INFO_NOT_REGISTERED)]
    for n_rows, pose, fin, fout in cases:
        rec = M.probe_record(acc, n_rows, (60, 300), pose, unobserved=77.0, flags=fin)
        want = M.record(acc, n_rows, (60, 300), pose, unobserved=77.0, flags=fin)
        assert rec["flags"] == fout == want["flags"]
        compare(rec, want, str((n_rows, fout)))
        assert rec["rank"] == 0 and not rec["H"].any() and np.array_equal(rec["cov_tangent"], 77.0 * np.eye(6))
    assert M.probe_record(acc, (3, 3), (60, 300), ok_pose)["flags"] == 0  # n = 6 is not flagged


def test_variances_floor():
    rec = np.zeros(1, REG_INFO)
    rec["var_tangent"][0] = [1e-9, 2.0, 1e4, 5e-5, 1e-3, 0.5]
    floor = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
    assert np.array_equal(api.reg_info_variances(rec[0], floor), [1e-6, 2.0, 1e4, 1e-4, 1e-3, 0.5])
    assert np.array_equal(api.reg_info_variances(rec[0]), rec["var_tangent"][0])
    out = np.zeros(6)
    assert api.lib().fbr_reg_info_variances(None, None, out.ctypes.data) == -1
    assert api.lib().fbr_reg_info_variances(rec.ctypes.data, None, None) == -1


# ------------------------------------------------------------------------------------ ABI
def test_symbols_sizes_and_defaults(tmp_path):
    src = open(os.path.join(REPO, "include", "fbr.h")).read()
    for s in ("fbr_info_params_default", "fbr_reg_info_poses", "fbr_batch_info", "fbr_reg_info_variances"):
        assert s in api.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % s, src), s
    assert api.lib().fbr_abi_version() == 4  # additions only
    assert "k_reg_info.hip" in build.HIP_SOURCES and "fbr_reg_info.hip" in build.HIP_SOURCES
    assert ctypes.sizeof(FbrInfoParams) == 48 and REG_INFO.itemsize == 1336
    for name, v in (("FBR_INFO_NO_ROWS", 1), ("FBR_INFO_FEW_ROWS", 2), ("FBR_INFO_BAD_POSE", 4), ("FBR_INFO_NOT_REGISTERED", 8)):
        assert "#define %s %d\n" % (name, v) in src
    p = FbrInfoParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    api.lib().fbr_info_params_default(ctypes.byref(p))
    assert bytes(p) == bytes(info_params())
    assert (p.eig_floor, p.unobserved_variance, p.sigma2, p.pose_chunk) == (100.0, 1e4, 0.0, 0)
    for name in ("reg_info", "batch_info"):
        assert callable(getattr(api.Context, name))
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fbr.h"\n'
                    'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(fbr_info_params), sizeof(fbr_reg_info),\n'
                    '  offsetof(fbr_reg_info, var_tangent), offsetof(fbr_reg_info, n_rows)); return 0; }\n')
    import subprocess
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(prog)])
    got = subprocess.check_output([exe]).split()
    assert [int(v) for v in got] == [48, 1336, REG_INFO.fields["var_tangent"][1], REG_INFO.fields["n_rows"][1]]


# ------------------------------------------------------------------------------------ the search-edge cases
def test_lattice_cases_are_unambiguous_but_for_the_dropped_queries():
    """What tests/test_reg_info.py's search-edge test relies on: on knn_model.lattice_cases() the
    model's accepted set hangs on no comparison within 4 ulps of its threshold, except at the queries
    of info_cases.LATTICE_DROPPED, which that test leaves out."""
    _, mc, ms = C.lattice_map()
    found, kept = {}, 0
    for c in K.lattice_cases():
        r = M.rows_at(mc, ms, K.xyz_of(c["corner"]), K.xyz_of(c["surf"]), c["guess"], K.CROP_HALF)
        bad = M.ambiguous(mc, ms, r)
        if bad:
            found[c["name"]] = bad
        corner, surf = C.lattice_clouds(c)
        r2 = M.rows_at(mc, ms, K.xyz_of(corner), K.xyz_of(surf), c["guess"], K.CROP_HALF)
        assert M.ambiguous(mc, ms, r2) == [], c["name"]
        kept += int(r2["ok"].sum())
        assert len(corner) + len(surf) == len(c["corner"]) + len(c["surf"]) - len(bad)
    assert found == C.LATTICE_DROPPED, found
    assert sum(len(v) for v in found.values()) == 29 and kept > 500  # 29 of 4,977 queries; the rest keep their rows
