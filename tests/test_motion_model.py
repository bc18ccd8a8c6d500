"""The motion path on the host (include/fbr.h "Motion deskew"): csrc/fbr_motion.h through the host
probe against the float64 model, the entry points of csrc/fbr_odom.cpp against the model, the struct
layouts against the header, and the conditions the test-scan generator must meet.  No device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import motion_model as M
import pyoracle as O
from conftest import REPO, build_probe
from feature_base_pointcloud_registration_amd import api, build, synth
from feature_base_pointcloud_registration_amd.fbr_types import (DESKEW_TABLE, GUESS_STATE, MOTION, ODOM_INFO, ODOM_SAMPLE,
                                                                default_params, ptr)

_F = ctypes.POINTER(ctypes.c_float)

# deskewPoint of a coordinate of size X = 100 m through two 3x3 products, in units of u = X * 2^-23
# (one float32 ulp of X is at most u, one rounding at most u / 2):
#   * entries of transFinal: six sinf / cosf (1/2 ulp each) through at most three roundings each, so
#     at most 4 * 2^-24 absolute per entry; the cofactor inverse doubles that: 8 * 2^-24;
#   * first product L = L1 * L2: three products of entries off by 8 and 4 (* 2^-24) and three
#     roundings: 16 * 2^-24 per entry of transBt;
#   * second product transBt * p: the entry errors against |p| <= X give 16 * sqrt(3) * 2^-24 * X
#     = 14 u; its three products and three sums round values up to sqrt(3) X + 6: 6 * 0.9 u = 5.3 u;
#   * the translation L1 * t2 + t1 (at most 3 sqrt(3) m per term) and pos = ratio * incre: < 1 u.
# 14 + 5.3 + 1 = 20.3 u, taken as 24 u.
TOL_100M = 24 * 100.0 * 2.0 ** -23
INCRE = (0.0, 0.0, 0.03, 1.0, 0.1, 0.0)  # the issue's motion of one 0.1-s scan at 10 m/s


@pytest.fixture(scope="module")
def probe():
    lib = build_probe("motion_probe")
    lib.mp_ratio_field.argtypes = [_F, ctypes.c_double, _F, ctypes.c_int64]
    lib.mp_ratio_column.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _F, ctypes.c_int64]
    lib.mp_deskew.argtypes = [_F, ctypes.c_int, ctypes.c_int, _F, _F, _F, _F, ctypes.c_int64]
    lib.mp_zero_t_pair.argtypes = [ctypes.c_float] * 3 + [_F, _F]
    return lib


def fp(a):
    return a.ctypes.data_as(_F)


def probe_deskew(lib, incre, flags, ratio_first, ratio, xyz):
    incre = np.ascontiguousarray(incre, np.float32)
    per_case = incre.ndim == 2
    rf = np.ascontiguousarray(np.atleast_1d(ratio_first), np.float32)
    ratio = np.ascontiguousarray(ratio, np.float32)
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros_like(xyz)
    lib.mp_deskew(fp(incre), flags, int(per_case), fp(rf), fp(ratio), fp(xyz), fp(out), len(xyz))
    return out


# ------------------------------------------------------------------------------- fbr_motion.h
def test_probe_matches_float64_model(probe):
    rng = np.random.default_rng(5)
    n = 2000
    incre = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(-3, 3, (n, 3))], 1).astype(np.float32)
    ratio = rng.uniform(0, 1, n).astype(np.float32)
    ratio[:50] = 0.0
    ratio[50:100] = np.float32(1.0) - np.float32(2.0 ** -24) * rng.integers(1, 4, 50).astype(np.float32)
    ratio[100:150] = np.float32(1799.0) / np.float32(1800.0)
    rfirst = rng.uniform(0, 1, n).astype(np.float32)
    rfirst[::3] = 0.0
    d = rng.normal(size=(n, 3))
    xyz = (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(1, 100, (n, 1))).astype(np.float32)
    xyz[:20] *= np.float32(100.0) / np.linalg.norm(xyz[:20].astype(np.float64), axis=1)[:, None].astype(np.float32)
    worst = 0.0
    for flags in (M.POSITION, M.POSITION | M.ROTATION, M.ROTATION):
        got = probe_deskew(probe, incre, flags, rfirst, ratio, xyz)
        want = np.stack([M.deskew(incre[i], flags, rfirst[i], ratio[i:i + 1], xyz[i:i + 1])[0] for i in range(n)])
        worst = max(worst, float(np.abs(got - want).max()))
    print("worst |probe - model| = %.3g m (bound %.3g)" % (worst, TOL_100M))
    assert worst <= TOL_100M


def test_zero_increment_returns_the_input_bits(probe):
    rng = np.random.default_rng(6)
    xyz = rng.uniform(-100, 100, (500, 3)).astype(np.float32)
    xyz[0] = (0.0, -1e-30, 1e-30)  # (-0 + 0 is +0 in deskewPoint's sums, as with a zero-rate IMU table)
    ratio = rng.uniform(0, 1, 500).astype(np.float32)
    for flags in (M.POSITION, M.POSITION | M.ROTATION):
        got = probe_deskew(probe, np.zeros(6, np.float32), flags, 0.25, ratio, xyz)
        assert np.array_equal(got.view(np.int32), xyz.view(np.int32))


def test_general_inverse_and_product_give_the_zero_translation_bits(probe):
    """affine_inverse_t / compose_t at t = +0 against fbr_imu.h's affine_inverse / compose."""
    rng = np.random.default_rng(7)
    for r, p, y in rng.uniform(-3.1, 3.1, (300, 3)):
        a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
        probe.mp_zero_t_pair(r, p, y, fp(a), fp(b))
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_ratios(probe):
    t = np.array([0.0, 1e-5, 0.05, 0.0999, 0.1], np.float32)
    out = np.zeros_like(t)
    probe.mp_ratio_field(fp(t), 0.1, fp(out), len(t))
    assert np.array_equal(out.view(np.int32), M.ratio_field32(t, 0.1).view(np.int32))
    for W, cf, d in ((1800, 900, 1), (1800, 0, -1), (900, 899, 1), (900, 450, -1)):
        col = np.arange(W, dtype=np.int32)
        out = np.zeros(W, np.float32)
        probe.mp_ratio_column(col.ctypes.data, cf, d, W, fp(out), W)
        assert np.array_equal(out.view(np.int32), M.ratio_column32(d, col, cf, W).view(np.int32))
        assert out[cf] == 0 and out.max() == np.float32(W - 1) / np.float32(W)
        assert out[(cf + d) % W] == np.float32(1) / np.float32(W)  # the column fired after the first


# ------------------------------------------------------------------------------- fbr_odom.cpp
def odom_queue(t0, t1, rate, rng, vel=(8.0, 0.5, 0.1), gyro=(0.02, -0.01, 0.3), scale=False):
    t = np.arange(t0, t1, 1.0 / rate)
    q = np.zeros(len(t), ODOM_SAMPLE)
    q["stamp"] = t
    q["position"] = (t - t0)[:, None] * np.asarray(vel)[None, :] + rng.normal(0, 1e-3, (len(t), 3)) + (3.0, -2.0, 1.0)
    for i, ti in enumerate(t):
        r, p, y = 0.01 + gyro[0] * (ti - t0), -0.02 + gyro[1] * (ti - t0), 0.7 + gyro[2] * (ti - t0)
        cy, sy, cp, sp, cr, sr = np.cos(y / 2), np.sin(y / 2), np.cos(p / 2), np.sin(p / 2), np.cos(r / 2), np.sin(r / 2)
        q["orientation"][i] = (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                               cr * cp * cy + sr * sp * sy)
    if scale:  # unnormalised orientations: tf::quaternionMsgToTF normalises them
        q["orientation"] *= rng.uniform(0.5, 1.5, (len(t), 1))
    q["covariance0"] = 3.0
    return q


def check_info(q, cur, nxt):
    info, n_pop = api.odom_deskew_info(q, cur, nxt)
    m = M.odom_deskew_info(q, cur, nxt)
    assert n_pop == m["n_pop"]
    assert info["odom_available"] == m["odom_available"] and info["odom_deskew_flag"] == m["odom_deskew_flag"]
    assert info["reset_id"] == m["reset_id"]
    # float results of double inputs of size <= 10: a float ulp, and the float pose algebra's few more
    assert np.allclose(info["initial_guess"], m["initial_guess"], rtol=0, atol=2e-6)
    assert np.allclose(info["motion"]["incre"], m["incre"], rtol=0, atol=1e-5)
    mo = info["motion"]
    assert mo["flags"] == 0 and mo["time_source"] == 0 and mo["column_direction"] == 1
    assert mo["scan_period"] == nxt - cur
    return info, m


@pytest.mark.parametrize("case", range(8))
def test_odom_deskew_info_matches_model(case):
    rng = np.random.default_rng(100 + case)
    rate = [200.0, 100.0, 400.0, 50.0][case % 4]
    cur = 50.0 + rng.uniform(0, 1)
    q = odom_queue(cur - rng.uniform(0.02, 0.3), cur + rng.uniform(0.12, 0.4), rate, rng, scale=case % 2 == 0)
    info, m = check_info(q, cur, cur + 0.1)
    assert m["n_pop"] == int(np.sum(q["stamp"] < cur - 0.01))
    if rate < 100.0 and not info["odom_available"]:  # 20 ms apart: no sample in [cur - 0.01, cur], :410-411
        assert q["stamp"][m["n_pop"]] > cur
        return
    assert info["odom_available"] == 1 and info["odom_deskew_flag"] == 1
    assert q["stamp"][m["start"]] >= cur and (m["start"] == 0 or q["stamp"][m["start"] - 1] < cur)
    assert np.linalg.norm(info["motion"]["incre"][3:]) == pytest.approx(0.1 * np.linalg.norm((8.0, 0.5, 0.1)), rel=0.1)


def test_odom_deskew_info_early_returns():
    rng = np.random.default_rng(9)
    q = odom_queue(9.9, 10.3, 200.0, rng)
    info, m = check_info(q[:0], 10.0, 10.1)                        # empty queue
    assert info["odom_available"] == 0 and m["n_pop"] == 0
    info, m = check_info(q[q["stamp"] < 9.98], 10.0, 10.1)          # every sample popped
    assert info["odom_available"] == 0 and m["n_pop"] == int(np.sum(q["stamp"] < 9.98))
    info, m = check_info(q[q["stamp"] > 10.0], 10.0, 10.1)          # front later than the scan
    assert info["odom_available"] == 0 and m["n_pop"] == 0
    info, m = check_info(q[q["stamp"] < 10.05], 10.0, 10.1)         # back earlier than the next scan
    assert info["odom_available"] == 1 and info["odom_deskew_flag"] == 0 and m["end"] is None
    assert not info["motion"]["incre"].any()
    late = q[q["stamp"] < 10.0]                                      # no stamp >= cur: the last sample
    info, m = check_info(late, 10.0, 10.1)
    assert m["start"] == len(late) - 1 and info["odom_available"] == 1 and info["odom_deskew_flag"] == 0
    assert info["initial_guess"][3] == np.float32(late["position"][-1][0])
    flip = q.copy()                                                  # the reset id changes inside the scan
    flip["covariance0"][flip["stamp"] > 10.05] = 4.0
    info, m = check_info(flip, 10.0, 10.1)
    assert info["odom_available"] == 1 and info["odom_deskew_flag"] == 0 and info["reset_id"] == 3
    assert m["end"] is not None
    half = q.copy()
    half["covariance0"] = 2.5                                        # round(): half away from zero
    assert api.odom_deskew_info(half, 10.0, 10.1)[0]["reset_id"] == 3


def test_motion_from_poses():
    rng = np.random.default_rng(11)
    for _ in range(50):
        prev = np.concatenate([rng.uniform(-0.2, 0.2, 2), rng.uniform(-3, 3, 1), rng.uniform(-20, 20, 3)])
        step = np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-1.5, 1.5, 3)])
        cur = M.pose(M.affine(prev) @ M.affine(step))
        m, guess = api.motion_from_poses(prev, cur, 0.1, 0.1, 0.1)
        # float32 poses of size <= 25 m decomposed and recomposed: a few ulps of 25 m
        assert np.allclose(m["incre"], step, rtol=0, atol=2e-5)
        assert m["flags"] == 3 and m["time_source"] == 0 and m["column_direction"] == 1 and m["scan_period"] == 0.1
        assert np.allclose(guess, M.pose(M.affine(cur) @ M.affine(step)), rtol=0, atol=4e-5)
        m2, g2 = api.motion_from_poses(prev, cur, 0.2, 0.1, 0.3)
        want_incre, want_guess = M.motion_from_poses(prev, cur, 0.2, 0.1, 0.3)
        assert np.allclose(m2["incre"], want_incre, rtol=0, atol=2e-5)
        assert np.allclose(g2, want_guess, rtol=0, atol=6e-5)
    p = np.zeros(6, np.float32)
    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(scan_period=0.0)):
        kw = dict(dt=0.1, scan_period=0.1, dt_next=0.1)
        kw.update(bad)
        with pytest.raises(api.FbrError) as e:
            api.motion_from_poses(p, p, **kw)
        assert e.value.status == -1
    with pytest.raises(api.FbrError):
        api.motion_from_poses(np.array([0, 0, 0, np.inf, 0, 0], np.float32), p, 0.1, 0.1, 0.1)


def test_update_initial_guess_branches_in_call_order():
    """Four scans as laserCloudInfoHandler runs them: the first frame from the IMU attitude, the
    odometry guess while the reset ids agree, the IMU increment once they differ, and a scan with
    neither (pose and state unchanged)."""
    rng = np.random.default_rng(12)
    q = odom_queue(9.9, 10.6, 100.0, rng)
    tabs = []
    for k in range(4):
        t = np.zeros(1, DESKEW_TABLE)[0]
        t["imu_available"] = 1 if k < 3 else 0
        t["imu_roll_init"], t["imu_pitch_init"], t["imu_yaw_init"] = 0.01 + 0.02 * k, -0.02 + 0.01 * k, 0.3 + 0.1 * k
        tabs.append(t)
    for heading in (0, 1):
        model, state = M.GuessModel(reset_id=3), None
        tr, want = np.zeros(6, np.float32), np.zeros(6)
        for k in range(4):
            info, _ = api.odom_deskew_info(q, 10.0 + 0.1 * k, 10.1 + 0.1 * k)
            if k >= 2:
                info["reset_id"] = 4  # the mapping side has not seen this reset yet
            if state is not None:
                state["reset_id"] = 3
            rpy = [tabs[k]["imu_roll_init"], tabs[k]["imu_pitch_init"], tabs[k]["imu_yaw_init"]]
            want = model.update(dict(odom_available=info["odom_available"], reset_id=info["reset_id"],
                                     initial_guess=info["initial_guess"].astype(np.float64)),
                                rpy, tabs[k]["imu_available"], k > 0, heading, want)
            before = None if state is None else state.copy()
            tr, state = api.update_initial_guess(state, info, tabs[k], k > 0, heading, tr)
            if k == 0:
                state["reset_id"] = 3
            assert np.allclose(tr, want, rtol=0, atol=2e-5), k
            assert np.allclose(state["last_imu"].reshape(3, 4), model.last[:3], rtol=0, atol=1e-6), k
            if k == 3:
                assert np.array_equal(state.view(np.uint8), before.view(np.uint8))
    tr0, _ = api.update_initial_guess(None, None, tabs[0], False, 0, np.ones(6, np.float32))
    assert tr0[2] == 0 and tr0[0] == tabs[0]["imu_roll_init"] and tr0[3] == 1  # the translation stays
    tr1, _ = api.update_initial_guess(None, None, None, True, 1, np.arange(6, dtype=np.float32))
    assert np.array_equal(tr1, np.arange(6, dtype=np.float32))


# ------------------------------------------------------------------------------- layout
def test_layout_matches_the_header(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fbr.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n",\n'
                   '  sizeof(fbr_motion), offsetof(fbr_motion, column_direction), offsetof(fbr_motion, incre),\n'
                   '  offsetof(fbr_motion, scan_period), sizeof(fbr_odom_sample), offsetof(fbr_odom_sample, orientation),\n'
                   '  offsetof(fbr_odom_sample, covariance0), sizeof(fbr_odom_info), offsetof(fbr_odom_info, initial_guess),\n'
                   '  offsetof(fbr_odom_info, reset_id), offsetof(fbr_odom_info, motion), sizeof(fbr_guess_state),\n'
                   '  offsetof(fbr_guess_state, last_imu), FBR_MOTION_POSITION, FBR_MOTION_ROTATION, FBR_TIME_FIELD,\n'
                   '  FBR_TIME_COLUMN);\n  return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["g++", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    from feature_base_pointcloud_registration_amd import fbr_types as T
    assert got == [MOTION.itemsize, MOTION.fields["column_direction"][1], MOTION.fields["incre"][1],
                   MOTION.fields["scan_period"][1], ODOM_SAMPLE.itemsize, ODOM_SAMPLE.fields["orientation"][1],
                   ODOM_SAMPLE.fields["covariance0"][1], ODOM_INFO.itemsize, ODOM_INFO.fields["initial_guess"][1],
                   ODOM_INFO.fields["reset_id"][1], ODOM_INFO.fields["motion"][1], GUESS_STATE.itemsize,
                   GUESS_STATE.fields["last_imu"][1], T.FBR_MOTION_POSITION, T.FBR_MOTION_ROTATION, T.FBR_TIME_FIELD,
                   T.FBR_TIME_COLUMN]
    assert MOTION.itemsize == 48
    lib = api.lib()
    for s in ("fbr_odom_deskew_info", "fbr_motion_from_poses", "fbr_update_initial_guess", "fbr_set_motion"):
        assert hasattr(lib, s) and s in api.EXPORTED_SYMBOLS, s
    assert lib.fbr_abi_version() == 4  # additions only
    assert "fbr_odom.cpp" in build.HOST_SOURCES


# ------------------------------------------------------------------------------- the generator
def static_scan(seed, H=16, W=1800):
    gt, guess = synth.job(seed)
    return gt, guess, synth.scan(gt, H, W, seed=seed)


def test_generator_direction():
    """The synthetic scans sweep their columns in the +1 sense (column_direction of the tests)."""
    for seed, (H, W) in ((21, (16, 1800)), (22, (16, 900)), (23, (64, 1800))):
        _, _, pts = static_scan(seed, H, W)
        d, err = M.scan_direction(pts, W)
        assert d == 1 and err[1] < 1.0 / W and err[-1] > 0.1, err


@pytest.mark.parametrize("direction", [1, -1])
def test_generator_time_and_column_agree(direction):
    W = 1800
    _, _, pts = static_scan(21)
    sk, s, src = M.skew_scan(pts, INCRE, 0.1, W, direction)
    kept, col, _ = M.proj_model.keep_mask(sk, 16, W)
    i0, cf = M.first_kept(sk, 16, W)
    assert s[i0] == 0
    assert np.array_equal(M.column_k(direction, col, cf, W)[kept], np.round(s[kept] * W).astype(np.int64))
    # time = float32(s * period): the field's ratio is the column's to a float ulp of 1
    assert np.abs(M.ratio_field32(sk["time"], 0.1)[kept] - M.ratio_column32(direction, col, cf, W)[kept]).max() < 2e-7
    # the deskew inverts the generator: float64 model on the skewed scan against the static one
    P = np.stack([pts["x"], pts["y"], pts["z"]], 1)[src][kept].astype(np.float64)
    Q = np.stack([sk["x"], sk["y"], sk["z"]], 1)[kept].astype(np.float64)
    back = M.deskew(np.asarray(INCRE), M.POSITION | M.ROTATION, 0.0, s[kept][::20], Q[::20])
    assert np.abs(back - P[::20]).max() < 100 * 2.0 ** -22  # the float32 storage of q and p


def test_generator_self_check():
    """A condition on the generator, not a measurement: the skewed C1 scans of seeds 21-24,
    registered as they are by the oracle, end at least 20 times farther from ground truth than the
    static scans (measured with the un-iterated generator: 0.45 to 0.54 m against 5.9 to 8.2 mm)."""
    P = default_params(16, 1800)
    corner, surf = synth.config_map("C1")
    omap = O.Map(P, corner, surf)
    for seed in (21, 22, 23, 24):
        gt, guess, pts = static_scan(seed)
        sk = M.skew_scan(pts, INCRE, 0.1, 1800)[0]
        err = []
        for scan in (pts, sk):
            st = O.Stream(P)
            pose, stats = st.process_scan(omap, scan, 0.0, guess)
            err.append(float(np.linalg.norm(pose[3:] - gt[3:])))
        print("seed %d: static %.4f m, skewed %.4f m" % (seed, err[0], err[1]))
        assert err[1] >= 20 * err[0], (seed, err)
