"""IMU deskew path: imuConverter and deskewInfo/imuDeskewInfo on the host,
deskewPoint inside the device compaction, transformUpdate's IMU slerp in the GN finalize.

The reference ships this code but disables it (deskewInfo() commented out at
imageProjection.cpp:189-191); these tests run the path as it works with the call enabled, against
the oracle's restatement of the same reference lines.  Parity bars:
  * tables (imuDeskewInfo), converted samples (imuConverter): bit-exact host vs oracle;
  * ring/column indices, ranges and feature masks stay bit-exact (range comes from the raw point,
    rangeMat is written before deskewPoint, :633-635);
  * deskewed coordinates: bit-exact (the device carries glibc's sinf / cosf, fbr_sincosf.h); a
    zero-rate table is the identity;
  * registered pose: within 1e-4 m / 1e-4 rad (north_star).
"""
import os

import numpy as np
import pytest

import pyoracle as O
from conftest import REPO
from feature_base_pointcloud_registration_amd import api, synth
from feature_base_pointcloud_registration_amd.fbr_types import (DESKEW_TABLE, FBR_DESKEW_READY, FBR_DESKEW_WAIT_IMU,
                                                                IMU_EXTRINSICS, IMU_QUEUE, IMU_SAMPLE, POINT_XYZI,
                                                                PointCloud2, default_params)

POSE_TOL = 1e-4


def tbytes(t):
    return np.array(t, DESKEW_TABLE).reshape(1).view(np.uint8)


def rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scan_table(stamp, gyro=(0.04, -0.03, 0.5), seed=0, rate=200.0):
    q = synth.imu_queue(stamp - 0.05, stamp + 0.16, rate=rate, gyro=gyro, seed=seed)
    t, _ = api.imu_deskew_info(q, stamp, stamp + 0.1)
    assert t["status"] == FBR_DESKEW_READY and t["imu_available"] == 1
    return t


# ------------------------------------------------------------------------------- host (CPU)
@pytest.mark.parametrize("case", range(8))
def test_deskew_info_matches_oracle(case):
    rng = np.random.default_rng(case)
    rate = [200.0, 100.0, 400.0, 50.0][case % 4]
    tcur = 100.0 + rng.uniform(0, 1)
    q = synth.imu_queue(tcur - rng.uniform(0.0, 0.3), tcur + rng.uniform(0.1, 0.4), rate=rate,
                        gyro=rng.normal(0, 0.5, 3), seed=case)
    if case % 3 == 0:  # unnormalised orientations: tf::quaternionMsgToTF normalises them
        q["orientation"] *= rng.uniform(0.5, 1.5, (len(q), 1))
    prev = np.zeros(1, DESKEW_TABLE)[0]
    prev["imu_roll_init"], prev["imu_pitch_init"] = 0.25, -0.5
    a, na = api.imu_deskew_info(q, tcur, tcur + 0.1, previous=prev)
    b, nb, rc = O.imu_deskew_info(q, tcur, tcur + 0.1, previous=prev)
    assert rc == 0 and na == nb
    assert np.array_equal(tbytes(a), tbytes(b))


def test_deskew_info_gate_and_edges():
    q = synth.imu_queue(9.9, 10.3)
    t, n = api.imu_deskew_info(q[:0], 10.0, 10.1)                  # empty queue
    assert t["status"] == FBR_DESKEW_WAIT_IMU and n == 0 and t["imu_available"] == 0
    t, n = api.imu_deskew_info(q[q["stamp"] > 10.0], 10.0, 10.1)   # front later than the scan
    assert t["status"] == FBR_DESKEW_WAIT_IMU and n == 0
    t, n = api.imu_deskew_info(q[q["stamp"] < 10.05], 10.0, 10.1)  # back earlier than the next scan
    assert t["status"] == FBR_DESKEW_WAIT_IMU and n == 0
    t, n = api.imu_deskew_info(q, 10.0, 10.1)
    assert t["status"] == FBR_DESKEW_READY and n == int(np.sum(q["stamp"] < 10.0 - 0.01))
    assert t["imu_pointer_cur"] == int(np.sum((q["stamp"] >= 9.99) & (q["stamp"] <= 10.11))) - 1
    sparse = q[[0, len(q) - 1]].copy()                              # one sample in the window
    sparse["stamp"] = [9.995, 10.2]
    t, _ = api.imu_deskew_info(sparse, 10.0, 10.1)
    assert t["status"] == FBR_DESKEW_READY and t["imu_available"] == 0
    dense = synth.imu_queue(9.99, 10.2, rate=5000.0)                # > queueLength samples in the window
    with pytest.raises(api.FbrError) as e:
        api.imu_deskew_info(dense, 10.0, 10.1)
    assert e.value.status == -4


def test_imu_convert_matches_oracle():
    rng = np.random.default_rng(3)
    for k in range(50):
        ext = np.zeros(1, IMU_EXTRINSICS)
        ext["ext_rot"] = rand_rot(rng).reshape(1, 9) if k % 2 else np.array([[-1, 0, 0, 0, 1, 0, 0, 0, -1.0]])
        ext["ext_rpy"] = rand_rot(rng).reshape(1, 9) if k % 3 else np.array([[0, 1, 0, -1, 0, 0, 0, 0, 1.0]])
        s = synth.imu_queue(0.0, 0.05, gyro=rng.normal(0, 1, 3), seed=k)
        a = api.imu_convert(ext, s)
        b, rc = O.imu_convert(ext, s)
        assert rc == [0] * len(s)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.allclose(a["angular_velocity"], s["angular_velocity"] @ ext["ext_rot"].reshape(3, 3).T)
    bad = np.zeros(1, IMU_SAMPLE)  # all-zero orientation: "please use a 9-axis IMU" (utility.h:246-250)
    with pytest.raises(api.FbrError):
        api.imu_convert(ext, bad)


def test_oracle_zero_rate_deskew_is_identity():
    P = default_params(16, 1800)
    gt, _ = synth.job(3)
    pts = synth.scan(gt, 16, 1800, seed=3)
    t = scan_table(5.0, gyro=(0.0, 0.0, 0.0))
    t["imu_rot_x"] = t["imu_rot_y"] = t["imu_rot_z"] = 0.0
    a, b = O.project(P, pts), O.project(P, pts, deskew=t)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def _rot(r, p, y):
    A, B, C, D, E, F = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    return np.array([[A * C, A * D * F - B * E, B * F + A * D * E], [B * C, A * E + B * D * F, B * D * E - A * F],
                     [-D, C * F, C * E]])


def test_oracle_deskew_geometry():
    """deskewPoint moves each kept point by R(t_first)^-1 R(t) (double-precision model)."""
    P = default_params(16, 1800)
    gt, _ = synth.job(4)
    pts = synth.scan(gt, 16, 1800, seed=4)
    stamp = 7.0
    t = scan_table(stamp, gyro=(0.1, -0.2, 1.5))
    raw, dsk = O.project(P, pts), O.project(P, pts, deskew=t)
    assert np.array_equal(raw["range"].view(np.int32), dsk["range"].view(np.int32))
    idx = {(float(p["x"]), float(p["y"]), float(p["z"])): i for i, p in enumerate(pts)}
    src = np.array([idx[(float(c["x"]), float(c["y"]), float(c["z"]))] for c in raw["cloud"]])
    n = t["imu_pointer_cur"]
    tt, rx, ry, rz = t["imu_time"][:n + 1], t["imu_rot_x"][:n + 1], t["imu_rot_y"][:n + 1], t["imu_rot_z"][:n + 1]

    def rot_at(rel):
        pt = stamp + rel
        return _rot(np.interp(pt, tt, rx), np.interp(pt, tt, ry), np.interp(pt, tt, rz))

    R0 = rot_at(float(pts["time"][src.min()]))
    xyz = np.stack([raw["cloud"][k].astype(np.float64) for k in "xyz"], 1)
    got = np.stack([dsk["cloud"][k].astype(np.float64) for k in "xyz"], 1)
    for j in range(0, len(src), 97):
        exp = R0.T @ rot_at(float(pts["time"][src[j]])) @ xyz[j]
        assert np.abs(exp - got[j]).max() < 1e-4
    assert np.abs(got - xyz).max() > 0.05  # the deskew actually moved points (1.5 rad/s over 0.1 s)


# ------------------------------------------------------------------------------- device (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed", [("C1", 11), ("C2", 12)])
def test_deskew_projection_matches_oracle(cfg, seed):
    H, W = synth.CONFIGS[cfg][:2]
    P = default_params(H, W)
    gt, _ = synth.job(seed)
    pts = synth.scan(gt, H, W, seed=seed)
    t = scan_table(20.0, gyro=(0.08, -0.05, 0.9), seed=seed)
    with api.Context(P) as ctx:
        ctx.set_deskew([t])
        g = ctx.project(pts)
        o = O.project(P, pts, deskew=t)
        for k in ["start_ring", "end_ring", "col_ind", "range"]:
            assert np.array_equal(g[k].view(np.uint8), o[k].view(np.uint8)), k
        assert np.array_equal(g["cloud"].view(np.uint8), o["cloud"].view(np.uint8))
        raw = ctx.project(pts[:0])  # ...deskew of an empty scan is a no-op
        assert len(raw["col_ind"]) == 0
        z = t.copy()
        z["imu_rot_x"] = z["imu_rot_y"] = z["imu_rot_z"] = 0.0
        ctx.set_deskew([z])  # zero rotation: bit-exact identity
        g0 = ctx.project(pts)
        o0 = O.project(P, pts)
        assert np.array_equal(g0["cloud"].view(np.uint8), o0["cloud"].view(np.uint8))
        ctx.set_deskew(None)  # back to the reference's runtime path
        assert np.array_equal(ctx.project(pts)["cloud"].view(np.uint8), o0["cloud"].view(np.uint8))


@pytest.mark.gpu
def test_deskew_stream_process_scan_matches_oracle():
    H, W = synth.CONFIGS["C1"][:2]
    P = default_params(H, W)
    cmap, smap = synth.config_map("C1")
    m = O.Map(P, cmap, smap)
    st = O.Stream(P)
    traj = synth.trajectory(9, 4)
    _, pose = synth.job(9)
    po, pg = pose.copy(), pose.copy()
    with api.Context(P) as ctx:
        ctx.set_map(cmap, smap)
        for k, gtk in enumerate(traj):
            stamp = 30.0 + 0.2 * k
            pts = synth.scan(gtk, H, W, seed=90 + k)
            t = scan_table(stamp, gyro=(0.05, 0.02, 0.4 + 0.1 * k), seed=k)
            t["imu_roll_init"], t["imu_pitch_init"] = gtk[0] + 0.01, gtk[1] - 0.01
            ctx.set_deskew([t])
            st.set_deskew(t)
            po, so = st.process_scan(m, pts, stamp, po)
            pg, sg = ctx.process_scan(pts, stamp, pg)
            assert sg["status"] == so["status"] == 0
            assert (sg["n_points"], sg["n_corner"], sg["n_surf"]) == (so["n_points"], so["n_corner"], so["n_surf"])
            assert (sg["iterations"], sg["n_sel"]) == (so["iterations"], so["n_sel"])
            assert np.abs(pg[3:] - po[3:]).max() <= POSE_TOL, (pg, po)
            assert np.abs(np.angle(np.exp(1j * (pg[:3].astype(np.float64) - po[:3])))).max() <= POSE_TOL


@pytest.mark.gpu
def test_deskew_imu_update_only_register():
    """fbr_register with an imuAvailable table applies transformUpdate's slerp (:1447-1474)."""
    d = np.load(os.path.join(REPO, "tests", "golden", "reg_small.npz"))
    P = default_params(16, 900)
    t = scan_table(1.0)
    t["imu_roll_init"], t["imu_pitch_init"] = 0.2, -0.3
    m = O.Map(P, d["corner_map"], d["surf_map"])
    po, so, _ = m.register(d["corner"], d["surf"], d["guess"], deskew=t)
    pn, _, _ = m.register(d["corner"], d["surf"], d["guess"])
    with api.Context(P) as ctx:
        ctx.set_map(d["corner_map"], d["surf_map"])
        ctx.set_deskew([t])
        pg, sg = ctx.register(d["corner"], d["surf"], d["guess"])
    assert np.abs(pg.astype(np.float64) - po).max() <= POSE_TOL
    assert abs(po[0] - pn[0]) > 1e-3  # the slerp moved roll towards imuRollInit
    assert np.array_equal(po[2:], pn[2:])


@pytest.mark.gpu
def test_deskew_batch_per_job_tables():
    H, W = synth.CONFIGS["C2"][:2]
    cmap, smap = synth.config_map("C2")
    P = default_params(H, W, max_batch=6)
    m = O.Map(P, cmap, smap)
    jobs = synth.make_jobs("C2", 6, base_seed=300)
    tabs = np.zeros(6, DESKEW_TABLE)
    for j in (0, 2, 5):  # jobs 1, 3, 4 stay on the reference's runtime path
        tabs[j] = scan_table(40.0 + j, gyro=(0.02, 0.03, 0.6), seed=j)
    with api.Context(P) as ctx:
        ctx.set_map(cmap, smap)
        ctx.set_deskew(tabs)
        poses, stats = ctx.process_batch([j[0] for j in jobs], np.stack([j[1] for j in jobs]))
    for j, (pts, guess, gt) in enumerate(jobs):
        s = O.Stream(P)
        s.set_deskew(tabs[j] if tabs[j]["imu_available"] else None)
        po, so = s.process_scan(m, pts, 0.0, guess)
        assert stats["status"][j] == 0 and stats["n_corner"][j] == so["n_corner"]
        assert (stats["iterations"][j], stats["n_sel"][j]) == (so["iterations"], so["n_sel"])
        assert np.abs(poses[j][3:] - po[3:]).max() <= POSE_TOL
        assert np.abs(np.angle(np.exp(1j * (poses[j][:3].astype(np.float64) - po[:3])))).max() <= POSE_TOL


@pytest.mark.gpu
def test_deskew_skipped_without_time_field():
    """A PointCloud2 without "time": deskewFlag = -1, deskewPoint returns the point (:548)."""
    H, W = 16, 1800
    P = default_params(H, W)
    gt, _ = synth.job(13)
    pts = synth.scan(gt, H, W, seed=13)
    rec = np.zeros(len(pts), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"),
                                       ("ring", "<u2")]))
    for k in rec.dtype.names:
        rec[k] = pts[k]
    with api.Context(P) as ctx:
        ctx.set_deskew([scan_table(3.0)])
        a = ctx.project_msg(PointCloud2.from_array(rec))
        b = O.project(P, pts)
    assert a["msg_flags"] & 1
    assert np.array_equal(a["cloud"].view(np.uint8), b["cloud"].view(np.uint8))


@pytest.mark.gpu
def test_deskew_tables_after_a_record_stage_require_restaging():
    """A batch staged without deskew tables lives on the device as 16-B records (no time field);
    giving it deskew tables afterwards makes fbr_batch_launch report FBR_ERR_STATE, and staging it
    again (24-B scans, with time) deskews it like fbr_process_batch with the same tables."""
    H, W = synth.CONFIGS["C2"][:2]
    cmap, smap = synth.config_map("C2")
    jobs = synth.make_jobs("C2", 2, base_seed=310)
    scans, guesses = [j[0] for j in jobs], np.stack([j[1] for j in jobs])
    tabs = np.zeros(2, DESKEW_TABLE)
    tabs[0] = scan_table(41.0, gyro=(0.02, 0.03, 0.6), seed=0)
    with api.Context(default_params(H, W, max_batch=2)) as ctx:
        ctx.set_map(cmap, smap)
        ctx.batch_stage(scans, guesses)
        ctx.set_deskew(tabs)
        with pytest.raises(Exception):
            ctx.batch_launch()
        ctx.batch_stage(scans, guesses)
        ctx.batch_launch()
        ctx.batch_wait()
        p1, s1 = ctx.batch_results()
        p2, s2 = ctx.process_batch(scans, guesses)
    assert np.array_equal(p1.view(np.int32), p2.view(np.int32)) and s1.tobytes() == s2.tobytes()


# ------------------------------------------------------------------------------- find_rotation's edges
# deskew_point / find_rotation on the device (k_compact<true>) where the in-order synthetic scans
# above never go: point times before the first IMU sample, exactly on samples, on and past the last
# one; tables of two samples and of nearly queueLength; transStartInverse from a first deskewed
# point that is not input point 0.  The shapes add a single ring, ragged row blocks and W = 4000.
EDGE_SHAPES = [(16, 1800), (1, 1800), (40, 1800), (6, 4000)]
EDGE_TABLES = {"two-samples": 1, "twenty": 20, "near-capacity": IMU_QUEUE - 2}  # imu_pointer_cur
EDGE_TCUR = 20.0
BRANCHES = ["before_first", "on_sample", "between", "on_last", "past_last"]


def edge_sample_times(cur):
    """Relative times of the table's cur + 1 samples, as float32: EDGE_TCUR + the value is exact in
    double, so a point whose float `time` is one of them lies exactly on that sample."""
    s = np.linspace(0.0125, 0.09, cur + 1).astype(np.float32)
    assert (np.diff(s) > 0).all() and ((EDGE_TCUR + s.astype(np.float64)) - EDGE_TCUR == s.astype(np.float64)).all()
    return s


def edge_table(cur):
    """A deskewInfo table written by hand: imuTime on edge_sample_times, imuRot a smooth rotation
    from 0 (imuDeskewInfo starts its integration at zero, :355-360)."""
    s = edge_sample_times(cur).astype(np.float64)
    t = np.zeros(1, DESKEW_TABLE)[0]
    t["status"], t["imu_available"], t["imu_pointer_cur"] = FBR_DESKEW_READY, 1, cur
    t["imu_roll_init"], t["imu_pitch_init"], t["imu_yaw_init"] = 0.01, -0.02, 0.3
    t["time_scan_cur"] = EDGE_TCUR
    t["imu_time"][:cur + 1] = EDGE_TCUR + s
    d = s - s[0]
    t["imu_rot_x"][:cur + 1] = 0.4 * d + 0.8 * d * d
    t["imu_rot_y"][:cur + 1] = -0.3 * d
    t["imu_rot_z"][:cur + 1] = 1.5 * d + 0.01 * np.sin(300.0 * d)
    return t


def find_rotation_branch(t, point_time):
    """findRotation (imageProjection.cpp:494-526) restated: which of its cases a point time takes."""
    cur, imu_time = int(t["imu_pointer_cur"]), t["imu_time"]
    front = 0
    while front < cur:
        if point_time < imu_time[front]:
            break
        front += 1
    if point_time > imu_time[front] or front == 0:
        return "before_first" if front == 0 else "past_last"
    if point_time == imu_time[front]:
        return "on_last"  # the loop ran out: interpolation with ratioFront = 1
    return "on_sample" if point_time == imu_time[front - 1] else "between"


def edge_times(n, cur, seed):
    """Point times (float32, relative) that take every case of find_rotation."""
    rng = np.random.default_rng(seed)
    s = edge_sample_times(cur)
    kind = rng.integers(0, 8, n)
    out = rng.uniform(s[0], s[-1], n).astype(np.float32)                     # between samples
    out = np.where(kind == 0, rng.uniform(-0.002, s[0], n).astype(np.float32), out)  # before the first
    out = np.where((kind == 1) | (kind == 2), s[rng.integers(0, cur, n)], out)       # on a sample
    out = np.where(kind == 3, s[-1], out)                                            # on the last
    out = np.where(kind == 4, rng.uniform(s[-1], 0.11, n).astype(np.float32), out)   # past it
    out[::97] = 0.0
    return out.astype(np.float32)


def _one_ring(pts):
    pts = pts[pts["ring"] == 9].copy()
    pts["ring"] = 0
    return pts


def edge_scan_variants(H, W, cur):
    """The scan in firing order, shuffled, and with its first points rejected by each gate (ring out
    of range, range < 1, NaN); intensity = input index.  In the last two the first point deskewPoint
    sees is not input point 0 and, with more rings than one, not on ring 0."""
    import proj_model as M
    gt, _ = synth.job(17)
    base = _one_ring(synth.scan(gt, 16, W, seed=17)) if H == 1 else synth.scan(gt, H, W, seed=17)
    base["time"] = edge_times(len(base), cur, seed=H * 10000 + W + cur)

    def first_late_ring(p, start):
        kept, _, _ = M.keep_mask(p, H, W)
        ok = kept & ((p["ring"] != 0) | (H == 1))
        ok[:start] = False
        return int(np.flatnonzero(ok)[0])

    shuffled = base[np.random.default_rng(cur).permutation(len(base))].copy()
    shuffled["ring"][:first_late_ring(shuffled, 1)] = 65535
    lead = base.copy()
    j = first_late_ring(lead, 3 * H + 5)
    gate = np.arange(j) % 3
    lead["ring"][:j][gate == 0] = H
    for k in "xyz":
        lead[k][:j][gate == 1] *= np.float32(0.01)
    lead["x"][:j][gate == 2] = np.nan
    out = {"in-order": base, "shuffled": shuffled, "leading-rejected": lead}
    for p in out.values():
        p["intensity"] = np.arange(len(p))
    return out


@pytest.mark.parametrize("H,W", EDGE_SHAPES)
@pytest.mark.parametrize("name", list(EDGE_TABLES))
def test_edge_scans_take_every_branch_of_find_rotation(H, W, name):
    cur = EDGE_TABLES[name]
    t = edge_table(cur)
    P = default_params(H, W)
    for variant, pts in edge_scan_variants(H, W, cur).items():
        o = O.project(P, pts, deskew=t)
        own = o["cloud"]["intensity"].astype(np.int64)  # the kept points: those deskewPoint sees
        times = EDGE_TCUR + pts["time"][own[::4]].astype(np.float64)  # a quarter of them will do
        taken = [find_rotation_branch(t, x) for x in times.tolist()]
        for b in BRANCHES:
            assert taken.count(b) > 0, (variant, b)
        on = {x for x, b in zip(times.tolist(), taken) if b == "on_sample"}
        assert len(on) >= min(cur, 3), variant  # exactly on several samples
        assert np.abs(np.stack([o["cloud"][k] for k in "xyz"]) -
                      np.stack([O.project(P, pts)["cloud"][k] for k in "xyz"])).max() > 1e-3  # and it moves points
        if variant != "in-order":
            first = int(own.min())
            assert first > 0 and (H == 1 or pts["ring"][first] != 0), (variant, first)
            assert variant == "shuffled" or first >= 3 * H + 5  # deep in the input


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", EDGE_SHAPES)
def test_deskew_device_matches_oracle_at_find_rotation_edges(H, W):
    P = default_params(H, W)
    with api.Context(P) as ctx:
        for name, cur in EDGE_TABLES.items():
            t = edge_table(cur)
            ctx.set_deskew([t])
            for variant, pts in edge_scan_variants(H, W, cur).items():
                g, o = ctx.project(pts), O.project(P, pts, deskew=t)
                for k in ["start_ring", "end_ring", "col_ind", "range", "cloud"]:
                    assert np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8),
                                          np.ascontiguousarray(o[k]).view(np.uint8)), (name, variant, k)
