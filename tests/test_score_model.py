"""The pose-scoring model (tests/score_model.py) on the CPU: its correspondences against a float64
brute force, the structured world's 125 poses, the lattice generator, and the C-ABI additions
(symbols, structure sizes, defaults).  No GPU is needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_model as K
import sc_fixtures as SF
import score_model as S
from conftest import REPO
from feature_base_pointcloud_registration_amd import api, build
from feature_base_pointcloud_registration_amd.fbr_types import (POSE_SCORE, FbrPoseLattice, FbrScoreParams, pose_lattice,
                                                                 score_params)

NEW = ["fbr_score_params_default", "fbr_score_poses", "fbr_pose_search"]


def brute64(map_xyz, q, g2, box):
    """(nearest index, decided) per query in float64: decided where neither the choice of the nearest
    point nor its side of the gate can turn on float32 rounding.  A float32 d2 of non-negative terms
    (three differences, three squares, two sums, each rounded) is within 5 * 2^-24 of the exact one,
    relatively; 8 * 2^-24 is taken."""
    m = np.asarray(map_xyz, np.float64)
    keep = np.flatnonzero(np.all((map_xyz >= box[0]) & (map_xyz <= box[1]), axis=1))
    d = ((np.asarray(q, np.float64)[:, None, :] - m[keep][None, :, :]) ** 2).sum(2)
    two = np.partition(d, 1, axis=1)[:, :2]
    eps = 8 * 2.0 ** -24
    decided = (two[:, 1] - two[:, 0] > 2 * eps * two[:, 1]) & (np.abs(two[:, 0] - float(g2)) > eps * float(g2))
    idx = keep[d.argmin(1)]
    return np.where(two[:, 0] < float(g2), idx, -1), decided


def test_model_correspondences_equal_a_float64_brute_force():
    """structured_case at its gt, at its guess and at the worst of the 125 poses, both maps: every
    decided query has the float64 nearest point (or none, beyond the gate).  Measured: 0 of 2,082
    queries undecided (0 %); the cap is 1 %."""
    R = S.structured_reference()
    s = R["case"]
    g2 = S.gate2(1.0)
    n = n_undecided = 0
    for pose in (s["gt"], s["guess"], R["poses"][R["order"][-1]]):
        T = S.affine32(pose)
        h = np.asarray(S.STRUCT_CROP_HALF, np.float32)
        box = ((-h) + T[:, 3], h + T[:, 3])
        _, keys = S.score(K.xyz_of(s["corner_map"]), K.xyz_of(s["surf_map"]), K.xyz_of(s["corner"]), K.xyz_of(s["surf"]), T,
                          S.STRUCT_CROP_HALF)
        nc = len(s["corner"])
        for m, p, kk in ((s["corner_map"], s["corner"], keys[:nc]), (s["surf_map"], s["surf"], keys[nc:])):
            want, decided = brute64(K.xyz_of(m), K.associate(T.reshape(12), K.xyz_of(p)), g2, box)
            got = np.where(kk == S.NONE, -1, (kk & np.uint64(0xFFFFFFFF)).astype(np.int64))
            assert np.array_equal(got[decided], want[decided])
            n += len(kk)
            n_undecided += int((~decided).sum())
    print("undecided", n_undecided, "of", n)
    assert n > 2000 and n_undecided <= 0.01 * n


def test_structured_case_gt_is_the_strict_minimum_of_125_poses():
    """The figures of the float64 KD-tree check that motivated the feature: 0.03738 at gt, 0.04280
    next, 0.2407 worst."""
    R = S.structured_reference()
    f, o = R["records"]["fitness"], R["order"]
    assert len(f) == 125 and np.array_equal(R["poses"][o[0]], R["case"]["gt"]) and o[0] == 62
    assert f[o[0]] < f[o[1]] and len(np.unique(f)) == 125
    assert abs(f[o[0]] - 0.03738) < 5e-6 and abs(f[o[1]] - 0.04280) < 5e-6 and abs(f[o[-1]] - 0.2407) < 5e-5
    assert (R["records"]["n"] == (len(R["case"]["corner"]), len(R["case"]["surf"]))).all()
    assert np.array_equal(o, sorted(range(125), key=lambda i: (f[i], i)))


def test_record_arithmetic_and_the_truncated_mean():
    g2 = S.gate2(0.5)
    assert g2 == np.float32(0.25)
    d = np.float32([0.0, 0.125, 0.2499])
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64([7, 3, 9])
    keys = np.concatenate([keys[:1], [S.NONE], keys[1:], [S.NONE, S.NONE]])
    r = S.record(2, keys, g2)
    assert list(r["n"]) == [2, 4] and list(r["n_in"]) == [1, 2]
    assert r["sum_d2"][0] == 0.0 and r["sum_d2"][1] == float(d[1]) + float(d[2])
    assert r["fitness"] == ((0.0 + r["sum_d2"][1]) + 3 * 0.25) / 6
    assert S.record(0, np.zeros(0, np.uint64), g2)["fitness"] == np.finfo(np.float64).max
    # a tie goes to the lower map index, the gate is strict, a non-finite query has no key
    m = np.float32([[1, 0, 0], [-1, 0, 0], [0, 0.5, 0]])
    q = np.float32([[0, 0, 0], [0, -0.5, 0], [np.nan, 0, 0], [np.inf, 0, 0]])
    k = S.nn_keys(m, q, S.gate2(1.0))
    assert k[0] == (np.uint64(np.float32(0.25).view(np.uint32)) << np.uint64(32)) | np.uint64(2)
    assert k[1] == S.NONE and k[2] == S.NONE and k[3] == S.NONE  # d2 = 1.0 exactly is no inlier
    k = S.nn_keys(m[:2], q[:1], S.gate2(1.0))
    assert k[0] == S.NONE
    k = S.nn_keys(m[:2], q[:1] + np.float32([0, 2.0 ** -12, 0]), np.float32(1.5))
    assert k[0] & np.uint64(0xFFFFFFFF) == 0  # both at the same d2: index 0


def test_lattice_counts_and_order():
    seeds = np.float32([[0.1, 0.2, 0.3, 10, 20, 30], [0, 0, -1, -5, 5, 0]])
    lat = S.lattice(seeds, (1.0, 0.5, 0.0, 0.2), (0.5, 0.25, 0.3, 0.1))
    assert lat.shape == (2 * 5 * 5 * 1 * 5, 6) and lat.dtype == np.float32
    # x fastest, then y, (z,) yaw, then the seed; every axis ascending
    assert np.array_equal(lat[:5, 3], np.float32(10) + np.float32([-1, -0.5, 0, 0.5, 1]))
    assert (lat[:5, 4] == np.float32(20) + np.float32(-0.5)).all() and lat[5, 4] == np.float32(20) + np.float32(-0.25)
    assert (lat[:25, 2] == np.float32(0.3) + np.float32(-2) * np.float32(0.1)).all()
    assert lat[25, 2] == np.float32(0.3) + np.float32(-1) * np.float32(0.1)
    assert (lat[:125, :2] == seeds[0, :2]).all() and (lat[:125, 5] == 30).all() and (lat[125:, 5] == 0).all()
    assert np.array_equal(lat[62], seeds[0]) and np.array_equal(lat[125 + 62], seeds[1])
    # step = 0 or half = 0: the single offset 0
    assert np.array_equal(S.lattice(seeds[:1], (1.0, 0, 0, 0), (0.0, 1, 1, 1)), seeds[:1])
    # a half that is no multiple of the step: floor
    assert len(S.axis_offsets(0.99, 0.25)) == 7 and len(S.axis_offsets(1.0, 0.25)) == 9 and len(S.axis_offsets(0.2, 0.25)) == 1
    # the division is float32's: 0.8f / 0.1f is 8 exactly, in double it is 7.99999998
    assert len(S.axis_offsets(0.8, 0.1)) == 17 and np.floor(np.float64(np.float32(0.7)) / np.float64(np.float32(0.1))) == 6
    assert len(S.axis_offsets(0.7, 0.1)) == 2 * int(np.floor(np.float32(0.7) / np.float32(0.1))) + 1
    # the lattice of the relocalisation: 13 x 13 x 17 = 2,873
    assert len(S.lattice(seeds[:1], (3.0, 3.0, 0.0, 0.8), (0.5, 0.5, 0.0, 0.1))) == 2873
    # the cap: 2^20 hypotheses pass, one more does not
    assert len(S.lattice(np.zeros((1 << 20, 6)), (0, 0, 0, 0), (0, 0, 0, 0))) == S.SEARCH_MAX
    assert len(S.lattice(np.zeros((1 << 10, 6)), (511.5, 0, 0, 0), (1.0, 0, 0, 0))) == 1023 << 10
    with pytest.raises(ValueError):
        S.lattice(np.zeros(((1 << 20) + 1, 6)), (0, 0, 0, 0), (0, 0, 0, 0))
    with pytest.raises(ValueError):
        S.lattice(np.zeros((1 << 10, 6)), (512.0, 0, 0, 0), (1.0, 0, 0, 0))
    with pytest.raises(ValueError):
        S.lattice(np.zeros((1, 6)), (1.0, 1.0, 1.0, 1.0), (0.01, 0.01, 0.01, 0.01))
    with pytest.raises(ValueError):
        S.axis_offsets(-1.0, 0.5)
    assert list(S.order([0.5, 0.25, 0.5, 0.25, 0.1], 4)) == [4, 1, 3, 0] and len(S.order([1.0], 0)) == 0


@pytest.mark.parametrize("q", [1, 3])
def test_oracle_from_the_coarse_seed_misses_the_bound(q):
    """Why the feature is needed: the CPU oracle registered from a seed 2.2 m / -1.3 m / 0.63 rad off
    the truth of C1 query 1 ends 2.9 m and 0.64 rad off, unconverged (query 3, from -2.7 m / 1.2 m /
    -0.74 rad, likewise)."""
    pose, st = S.reloc_seed_oracle(q)
    dt, da = SF.pose_err(pose, SF.reloc()["queries"][q]["gt"])
    print("seed registration error", dt, da, st["converged"])
    assert dt > SF.RELOC_BOUND[0] and da > SF.RELOC_BOUND[1] and not st["converged"]


# ------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_exported_and_listed():
    lib = ctypes.CDLL(api.lib_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fbr.h")).read(), flags=re.S)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in api.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, src), s
    assert api.lib().fbr_abi_version() == 4  # additions only
    assert "k_score.hip" in build.HIP_SOURCES and "fbr_score.hip" in build.HIP_SOURCES


def test_structure_sizes_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fbr.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %lld\\n", sizeof(fbr_score_params), sizeof(fbr_pose_score),\n'
                   '  sizeof(fbr_pose_lattice), offsetof(fbr_score_params, pose_chunk), offsetof(fbr_pose_score, n_in),\n'
                   '  offsetof(fbr_pose_score, sum_d2), offsetof(fbr_pose_score, fitness), (long long)FBR_POSE_SEARCH_MAX);\n'
                   '  return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["g++", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(FbrScoreParams), POSE_SCORE.itemsize, ctypes.sizeof(FbrPoseLattice),
                   FbrScoreParams.pose_chunk.offset, POSE_SCORE.fields["n_in"][1], POSE_SCORE.fields["sum_d2"][1],
                   POSE_SCORE.fields["fitness"][1], S.SEARCH_MAX]
    assert got[:3] == [32, 40, 32] and S.SCORE == POSE_SCORE


def test_defaults_are_as_documented():
    p = FbrScoreParams(0.5, 7, 9, (1, 2, 3, 4, 5))
    api.lib().fbr_score_params_default(ctypes.byref(p))
    q = score_params()
    for name, _ in FbrScoreParams._fields_:
        a, b = getattr(p, name), getattr(q, name)
        assert (list(a) == list(b)) if name == "reserved_" else (a == b), name
    assert (p.gate, p.use_crop, p.pose_chunk, list(p.reserved_)) == (1.0, 1, 0, [0] * 5)
    lat = pose_lattice((3.0, 3.0, 0.0, 0.8), (0.5, 0.5, 0.0, 0.1))
    assert list(lat.half) == [3.0, 3.0, 0.0, np.float32(0.8)] and list(lat.step) == [0.5, 0.5, 0.0, np.float32(0.1)]
