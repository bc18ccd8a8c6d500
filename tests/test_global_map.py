"""The global map on the device (include/fbr.h "global map"): the wide VoxelGrid alone, a build in
the reference's mode and in the wide mode, the store's edge cases, install, save and resources.

Parity bars:
  * the wide kernel where PCL does not overflow: byte-equal to Context.voxel_grid (default order);
  * the wide kernel where PCL overflows: byte-equal to the NumPy model (tests/gmap_model.py);
  * a reference-mode build against the oracle's composition (transform in NumPy, O.voxel_grid):
    sizes and voxel order exact, centroids within MAP_ATOL = 2e-4 (PCL sums a voxel's points in
    std::sort's order), byte-equal on an exact_voxel_order context;
  * install against set_map(*global_map()): equal maps, grids and pose bits; the pose within
    POSE_TOL = 1e-4 of the oracle and 0.05 m of ground truth (tests/test_keyframes.py's bars);
  * save: the ASCII files carry 8 significant digits, so a value read back differs from the one
    written by at most half a unit of the eighth digit, 5e-8 relative (SAVE_RTOL = 1e-7 with margin).
"""
import os

import numpy as np
import pytest

import gmap_model as M
import pyoracle as O
from feature_base_pointcloud_registration_amd import api, synth
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
MAP_ATOL = 2e-4
SAVE_RTOL = 1e-7
FBR_ERR_STATE = -7


def make_keyframes(n, H=16, W=1800, seed=7, step=1.5):
    """tests/test_keyframes.py's recipe: n keyframes along a trajectory, GT key poses, the scans'
    DS'd corner / surf features."""
    P = default_params(H, W)
    traj = synth.trajectory(seed, n + 1, step=step)
    poses = np.zeros(n, KEYPOSE)
    corners, surfs = [], []
    for k in range(n):
        gt = traj[k]
        f = O.Stream(P).features(synth.scan(gt, H, W, seed=100 + k))
        corners.append(O.voxel_grid(f["corner"], P.mapping_corner_leaf_size))
        surfs.append(O.voxel_grid(f["surf"], P.mapping_surf_leaf_size))
        poses[k] = (gt[3], gt[4], gt[5], k, gt[0], gt[1], gt[2], 0.0, 2.0 * k)
    return P, poses, corners, surfs, traj[n]


def _transform(cloud, pose):
    m = O.affine_from_pose(np.array([pose["roll"], pose["pitch"], pose["yaw"], pose["x"], pose["y"], pose["z"]],
                                    np.float32))
    out = cloud.copy()
    for r, k in enumerate("xyz"):
        out[k] = m[r, 0] * cloud["x"] + m[r, 1] * cloud["y"] + m[r, 2] * cloud["z"] + m[r, 3]
    return out


def concat(clouds, poses):
    parts = [_transform(c, p) for c, p in zip(clouds, poses) if len(c)]
    return np.concatenate(parts) if parts else np.zeros(0, POINT_XYZI)


def same_bytes(a, b):
    return len(a) == len(b) and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _close_maps(a, b):
    assert len(a) == len(b)
    A, B = a.view(np.float32).reshape(-1, 4), b.view(np.float32).reshape(-1, 4)
    assert np.abs(A[:, :3] - B[:, :3]).max(initial=0) <= MAP_ATOL
    assert np.abs(A[:, 3] - B[:, 3]).max(initial=0) <= 1e-2


def _pose_close(p, q):
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    assert np.abs(p[3:] - q[3:]).max() <= POSE_TOL, (p, q)
    assert np.abs(np.angle(np.exp(1j * (p[:3] - q[:3])))).max() <= POSE_TOL, (p, q)


def fill(ctx, poses, corners, surfs):
    for k in range(len(poses)):
        ctx.keyframes_add(poses[k], corners[k], surfs[k])


@pytest.fixture(scope="module")
def kf10():
    return make_keyframes(10)


@pytest.fixture(scope="module")
def ref10(kf10):
    """The oracle's composition for the 10-keyframe store, computed once: (corner, surf)."""
    P, poses, corners, surfs, _ = kf10
    return (O.voxel_grid(concat(corners, poses), P.mapping_corner_leaf_size),
            O.voxel_grid(concat(surfs, poses), P.mapping_surf_leaf_size))


@pytest.fixture(scope="module")
def ctx():
    with api.Context(default_params(16, 1800)) as c:
        yield c


def random_cloud(n, seed, box=(20.0, 16.0, 4.0)):
    rng = np.random.default_rng(seed)
    out = np.zeros(n, POINT_XYZI)
    for d, k in enumerate("xyz"):
        out[k] = rng.uniform(-box[d] / 2, box[d] / 2, n).astype(np.float32)
    out["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    return out


# ---- 1. the wide kernel alone ----
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 32768, 65537])
def test_wide_kernel_equals_voxel_grid_where_pcl_does_not_overflow(ctx, n):
    pts = random_cloud(n, seed=n)
    for leaf in (0.4, 1.0):
        ref = ctx.voxel_grid(pts, leaf)
        got = ctx.selftest_voxel_wide(pts, leaf)
        assert 1 <= len(ref) <= n
        assert same_bytes(got, ref)
    assert n < 255 or len(ref) < n  # at the 1 m leaf some voxels hold several points


@pytest.mark.parametrize("n", [257, 65537])
def test_wide_kernel_one_voxel_and_one_point_per_voxel(ctx, n):
    rng = np.random.default_rng(n)
    one = np.zeros(n, POINT_XYZI)
    for k in "xyz":
        one[k] = rng.uniform(0.21, 0.39, n).astype(np.float32)
    one["intensity"] = rng.uniform(0, 10, n).astype(np.float32)
    ref = ctx.voxel_grid(one, 0.2)
    assert len(ref) == 1
    assert same_bytes(ctx.selftest_voxel_wide(one, 0.2), ref)
    own = np.zeros(n, POINT_XYZI)
    i = rng.permutation(n)
    own["x"], own["y"], own["z"] = (i % 64) * 0.5 + 0.1, ((i // 64) % 64) * 0.5 + 0.1, (i // 4096) * 0.5 + 0.1
    own["intensity"] = i
    ref = ctx.voxel_grid(own, 0.2)
    assert len(ref) == n
    assert same_bytes(ctx.selftest_voxel_wide(own, 0.2), ref)


@pytest.mark.parametrize("case", list(M.OVERFLOW_SEPS))
def test_wide_kernel_equals_the_model_on_overflow_clouds(ctx, case):
    pts = M.overflow_cloud(M.OVERFLOW_SEPS[case])
    assert same_bytes(ctx.voxel_grid(pts, 0.2), pts)  # PCL's semantics: "leaf size is too small", output = input
    want = M.voxel_grid_wide(pts, 0.2)
    got = ctx.selftest_voxel_wide(pts, 0.2)
    assert len(want) < len(pts)
    assert same_bytes(got, want)
    assert same_bytes(ctx.selftest_voxel_wide(pts, 0.2), got)  # two calls, the same bytes
    holed = pts.copy()
    holed["z"][17] = np.nan
    holed["x"][3000] = -np.inf
    assert same_bytes(ctx.selftest_voxel_wide(holed, 0.2), M.voxel_grid_wide(holed, 0.2))


def test_wide_kernel_refuses_what_it_cannot_key(ctx):
    pts = random_cloud(64, seed=1)
    far = pts.copy()
    far["x"] += np.float32(0.2 * 2**24 + 100.0)  # a bound of 2^24 cells or more
    with pytest.raises(api.FbrError) as e:
        ctx.selftest_voxel_wide(far, 0.2)
    assert e.value.status == -4
    huge = pts.copy()
    huge["x"][:32] -= 3.0e5
    huge["y"][:32] -= 3.0e5
    huge["z"][:32] -= 3.0e5
    huge["x"][32:] += 3.0e5
    huge["y"][32:] += 3.0e5
    huge["z"][32:] += 3.0e5  # 2^63 cells or more
    with pytest.raises(api.FbrError) as e:
        ctx.selftest_voxel_wide(huge, 0.2)
    assert e.value.status == -4
    assert len(ctx.selftest_voxel_wide(np.zeros(0, POINT_XYZI), 0.2)) == 0


# ---- 2. reference mode ----
def test_reference_mode_build_equals_the_oracle_composition(kf10, ref10):
    P, poses, corners, surfs, _ = kf10
    with api.Context(P) as c:
        with pytest.raises(api.FbrError) as e:  # no build yet
            c.global_map()
        assert e.value.status == FBR_ERR_STATE
        fill(c, poses, corners, surfs)
        r = c.global_map_build()
        gc, gs = c.global_map()
        assert (r["n_keyframes"], r["n_corner"], r["n_surf"], r["n_dropped"]) == (10, len(ref10[0]), len(ref10[1]), 0)
        assert (r["n_corner_raw"], r["n_surf_raw"]) == (sum(map(len, corners)), sum(map(len, surfs)))
        assert (r["corner_overflow"], r["surf_overflow"], r["corner_wide"], r["surf_wide"]) == (0, 0, 0, 0)
        _close_maps(gc, ref10[0])
        _close_maps(gs, ref10[1])
        # no overflow: the wide mode takes the normal path and returns the same bytes
        w = c.global_map_build(wide=1, keep_raw=1)
        wc, ws = c.global_map()
        assert (w["corner_wide"], w["surf_wide"]) == (0, 0)
        assert same_bytes(wc, gc) and same_bytes(ws, gs)
        # the map, the grids and the key poses are not touched
        with pytest.raises(api.FbrError) as e:
            c.get_map()
        assert e.value.status == -3


def test_reference_mode_is_byte_equal_with_exact_voxel_order(kf10, ref10):
    _, poses, corners, surfs, _ = kf10
    with api.Context(default_params(16, 1800, exact_voxel_order=1)) as c:
        fill(c, poses, corners, surfs)
        c.global_map_build()
        gc, gs = c.global_map()
    assert same_bytes(gc, ref10[0]) and same_bytes(gs, ref10[1])


# ---- 3. store edge cases ----
def test_store_edge_cases(kf10):
    P, poses, corners, surfs, _ = kf10
    lc, ls = P.mapping_corner_leaf_size, P.mapping_surf_leaf_size
    empty = np.zeros(0, POINT_XYZI)
    with api.Context(P) as c:
        r = c.global_map_build()  # no keyframes: FBR_OK, zeros
        assert all(v == 0 for v in r.values())
        assert [len(a) for a in c.global_map()] == [0, 0]
        # one keyframe only
        c.keyframes_add(poses[0], corners[0], surfs[0])
        r = c.global_map_build()
        gc, gs = c.global_map()
        _close_maps(gc, O.voxel_grid(_transform(corners[0], poses[0]), lc))
        _close_maps(gs, O.voxel_grid(_transform(surfs[0], poses[0]), ls))
        assert r["n_keyframes"] == 1
        # an empty corner cloud, a keyframe of exactly 256 points and one of 257
        cs = [corners[0], empty, corners[2][:256], corners[3][:257]]
        ss = [surfs[0][:257], surfs[1][:256], surfs[2], empty]
        assert len(cs[2]) == 256 and len(cs[3]) == 257 and len(ss[0]) == 257 and len(ss[1]) == 256
        c.keyframes_reset()
        fill(c, poses[:4], cs, ss)
        r = c.global_map_build(keep_raw=1)
        gc, gs = c.global_map()
        _close_maps(gc, O.voxel_grid(concat(cs, poses[:4]), lc))
        _close_maps(gs, O.voxel_grid(concat(ss, poses[:4]), ls))
        assert (r["n_keyframes"], r["n_corner_raw"], r["n_surf_raw"]) == (4, sum(map(len, cs)), sum(map(len, ss)))
        # a single NaN point is dropped and counted, and changes nothing else
        holed = [a.copy() for a in cs]
        holed[2] = np.insert(cs[2], 100, np.array([(np.nan, 1.0, 2.0, 3.0)], POINT_XYZI))
        c.keyframes_reset()
        fill(c, poses[:4], holed, ss)
        r = c.global_map_build(keep_raw=1)
        assert (r["n_dropped"], r["n_corner_raw"]) == (1, sum(map(len, cs)))
        hc, hs = c.global_map()
        assert same_bytes(hc, gc) and same_bytes(hs, gs)
        # a build after keyframes_set_pose on every keyframe follows the moved poses
        moved = poses[:4].copy()
        moved["x"] += 0.05
        moved["yaw"] += 0.002
        for k in range(4):
            c.keyframes_set_pose(k, moved[k])
        c.global_map_build()
        mc, ms = c.global_map()
        _close_maps(mc, O.voxel_grid(concat(cs, moved), lc))
        _close_maps(ms, O.voxel_grid(concat(ss, moved), ls))
        assert not same_bytes(mc, gc)


# ---- 4. overflow ----
def test_overflow_reference_and_wide_modes(kf10):
    P, poses, corners, surfs, _ = kf10
    lc, ls = P.mapping_corner_leaf_size, P.mapping_surf_leaf_size
    far = poses[:4].copy()
    far["x"][2:] += 2000.0
    far["y"][2:] += 2000.0
    far["z"][2:] += 200.0
    cs, ss = corners[:4], surfs[:4]
    raw_c, raw_s = concat(cs, far), concat(ss, far)
    g = M.cloud_grid(raw_c, lc)
    assert g["pcl_overflow"] == 1 and g["div_b"][0] * g["div_b"][1] * g["div_b"][2] > 2**32
    want_c, want_s = M.voxel_grid_wide(raw_c, lc), M.voxel_grid_wide(raw_s, ls)
    with api.Context(P) as c:
        fill(c, far, cs, ss)
        r = c.global_map_build(wide=0)
        gc, gs = c.global_map()
        assert (r["corner_overflow"], r["surf_overflow"], r["corner_wide"], r["surf_wide"]) == (1, 1, 0, 0)
        assert same_bytes(gc, raw_c) and same_bytes(gs, raw_s)  # PCL's semantics: the raw concatenation
        r = c.global_map_build(wide=1)
        wc, ws = c.global_map()
        assert (r["corner_overflow"], r["surf_overflow"], r["corner_wide"], r["surf_wide"]) == (1, 1, 1, 1)
        assert (r["n_corner"], r["n_surf"]) == (len(want_c), len(want_s))
        assert len(want_c) < len(raw_c) and len(want_s) < len(raw_s)
        assert same_bytes(wc, want_c) and same_bytes(ws, want_s)
        r2 = c.global_map_build(wide=1, keep_raw=1)  # again, keeping the raw clouds: the same bytes
        wc2, ws2 = c.global_map()
        assert r2 == r and same_bytes(wc2, wc) and same_bytes(ws2, ws)
    # a NaN point in the wide path
    holed = [a.copy() for a in cs]
    holed[1] = np.insert(cs[1], 7, np.array([(0.0, np.nan, 0.0, 1.0)], POINT_XYZI))
    with api.Context(P) as c:
        fill(c, far, holed, ss)
        r = c.global_map_build(wide=1)
        assert (r["n_dropped"], r["corner_wide"], r["n_corner_raw"]) == (1, 1, len(raw_c))
        assert same_bytes(c.global_map()[0], want_c)


# ---- 5. install ----
def test_install_equals_set_map_of_the_built_clouds(kf10):
    P, poses, corners, surfs, gt_next = kf10
    guess = np.asarray(gt_next, np.float32).copy()
    guess[:3] += np.float32([0.01, -0.01, 0.02])
    guess[3:] += np.float32([0.2, -0.15, 0.05])
    f = O.Stream(P).features(synth.scan(gt_next, 16, 1800, seed=999))
    with api.Context(P) as a, api.Context(P) as b:
        fill(a, poses, corners, surfs)
        a.global_map_build()
        gc, gs = a.global_map()
        a.global_map_install()
        b.set_map(gc, gs)
        assert a.map_grid_info() == b.map_grid_info()
        pa, sa = a.register(f["corner"], f["surf"], guess)
        pb, sb = b.register(f["corner"], f["surf"], guess)
        ma, mb = a.get_map(), b.get_map()
        assert same_bytes(ma[0], mb[0]) and same_bytes(ma[1], mb[1])
        assert np.array_equal(pa.view(np.int32), pb.view(np.int32)) and sa == sb
        # a later set_map replaces the installed map as usual
        a.set_map(gc[:100], gs[:100])
        assert len(a.get_map()[0]) <= 100
    po, so, _ = O.Map(P, gc, gs).register(f["corner"], f["surf"], guess)
    assert sa["status"] == so["status"] == 0
    _pose_close(pa, po)
    assert np.abs(pa[3:] - np.asarray(gt_next[3:], np.float32)).max() < 0.05


# ---- 6. save ----
def _close_saved(a, b):
    assert len(a) == len(b)
    A, B = a.view(np.float32).reshape(-1, 4).astype(np.float64), b.view(np.float32).reshape(-1, 4).astype(np.float64)
    assert (np.abs(A - B) <= SAVE_RTOL * np.abs(B)).all()


def test_save_writes_the_reference_files(kf10, tmp_path):
    P, poses, corners, surfs, _ = kf10
    with api.Context(P) as a, api.Context(P) as b:
        fill(a, poses, corners, surfs)
        with pytest.raises(api.FbrError) as e:
            a.global_map_save(str(tmp_path))
        assert e.value.status == FBR_ERR_STATE
        r = a.global_map_build(keep_raw=1)
        (tmp_path / "keep.txt").write_text("kept")
        a.global_map_save(str(tmp_path))
        assert sorted(os.listdir(tmp_path)) == ["cloudCorner.pcd", "cloudSurf.pcd", "keep.txt", "trajectory.pcd",
                                                "transformations.pcd"]
        a.global_map_save(str(tmp_path), cloud_global=True)
        assert (tmp_path / "keep.txt").read_text() == "kept"  # nothing is removed
        gc, gs = a.global_map()
        _close_saved(api.pcd_read(str(tmp_path / "cloudCorner.pcd")), gc)
        _close_saved(api.pcd_read(str(tmp_path / "cloudSurf.pcd")), gs)
        glob = api.pcd_read(str(tmp_path / "cloudGlobal.pcd"))
        assert len(glob) == r["n_corner_raw"] + r["n_surf_raw"]
        _close_saved(glob, np.concatenate([concat(corners, poses), concat(surfs, poses)]))
        # the localiser's start-up on the written files gives the installed map
        a.global_map_install()
        b.load_map(str(tmp_path / "cloudCorner.pcd"), str(tmp_path / "cloudSurf.pcd"))
        ma, mb = a.get_map(), b.get_map()
        _close_saved(mb[0], ma[0])
        _close_saved(mb[1], ma[1])
        traj = api.pcd_read(str(tmp_path / "trajectory.pcd"))
        want = np.zeros(len(poses), POINT_XYZI)
        for k in ("x", "y", "z", "intensity"):
            want[k] = poses[k]
        _close_saved(traj, want)
        assert np.array_equal(traj["intensity"], np.arange(len(poses), dtype=np.float32))
        rows = [ln.split() for ln in open(tmp_path / "transformations.pcd").read().split("DATA ascii\n")[1].splitlines()]
        assert len(rows) == len(poses) and all(len(row) == 8 for row in rows)
        assert [float(row[7]) for row in rows] == [float(t) for t in poses["time"]]
        with pytest.raises(api.FbrError) as e:
            a.global_map_save(str(tmp_path / "missing"))
        assert e.value.status == -1


# ---- 7. resources ----
def test_resources_return_and_reset_drops_the_map(kf10):
    P, poses, corners, surfs, _ = kf10
    before = api.live_resources()
    with api.Context(P) as c:
        fill(c, poses[:3], corners[:3], surfs[:3])
        c.global_map_build(wide=1, keep_raw=1)
        c.global_map_install()
        held = api.live_resources()
        c.keyframes_reset()
        assert api.live_resources()[0] == held[0] - 4  # the built and raw clouds are gone; the installed map stays
        with pytest.raises(api.FbrError) as e:
            c.global_map()
        assert e.value.status == FBR_ERR_STATE
        with pytest.raises(api.FbrError) as e:
            c.global_map_install()
        assert e.value.status == FBR_ERR_STATE
        assert len(c.get_map()[0]) > 0
        fill(c, poses[:3], corners[:3], surfs[:3])
        c.global_map_build()
    assert api.live_resources() == before
