"""Inputs of the keyframe local map tests (tests/test_kf_model.py on the CPU, tests/test_keyframe_map.py
on the device): the selection and launch-shape cases, and the sixteen-keyframe mapping loop.

A case is a dict: name, poses (KEYPOSE, intensity = key index), corners / surfs (one lidar-frame cloud
per keyframe), kp (keyword arguments of keyframe_params) and stamp.  `shape` says what the case is
meant to reach; test_kf_model.py asserts it on the model, so that a case cannot quietly degenerate.
"""
import functools

import numpy as np

from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params, keyframe_params

SEG_SIZES = (0, 1, 255, 256, 257, 16384, 16385, 40000)  # k_kf_transform: 256 lanes, 64 blocks per segment
N_MANY = 65537  # > 65535 selected entries: the second blockIdx.y chunk of launch_kf_transform
LOOP_KP = dict(search_radius=8.0, recent_window=3.0)
LOOP_N = 16
VG_LARGE_MIN = 32768  # voxel_grid_dev: the one-workgroup filter below, voxel_grid_large from here on


def params(exact=0):
    return default_params(16, 1800, exact_voxel_order=exact)


def cloud(rng, n, half=(3.0, 3.0, 1.0)):
    c = np.zeros(n, POINT_XYZI)
    for k, h in zip("xyz", half):
        c[k] = rng.uniform(-h, h, n).astype(np.float32)
    c["intensity"] = rng.uniform(0, 100, n).astype(np.float32)
    return c


def key_poses(xyz, times=None, rng=None):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(len(xyz), KEYPOSE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["intensity"] = np.arange(len(xyz), dtype=np.float32)
    p["time"] = np.arange(len(xyz), dtype=np.float64) if times is None else np.asarray(times, np.float64)
    if rng is not None:  # a rotation of its own per key, so that a wrong key's pose shows
        p["roll"] = rng.uniform(-0.1, 0.1, len(xyz)).astype(np.float32)
        p["pitch"] = rng.uniform(-0.1, 0.1, len(xyz)).astype(np.float32)
        p["yaw"] = rng.uniform(-3.0, 3.0, len(xyz)).astype(np.float32)
    return p


def _case(name, seed, xyz, kp, stamp, times=None, sizes=None, shape=None):
    rng = np.random.default_rng(seed)
    poses = key_poses(xyz, times, rng)
    n = len(poses)
    sizes = sizes if sizes is not None else [(30 + k, 60 + k) for k in range(n)]  # the map size names the key
    return dict(name=name, poses=poses, corners=[cloud(rng, a) for a, _ in sizes], surfs=[cloud(rng, b) for _, b in sizes],
                kp=kp, stamp=float(stamp), shape=shape or {})


def _segment_sizes():
    # (corner, surf) per keyframe: every size of SEG_SIZES on the surf side (73 k points: voxel_grid_large), the
    # sizes up to 257 and 16385 on the corner side (17 k points: the one-workgroup filter); keyframes 6 and 8 are empty in corner only, 7 in both; the last three have no corner
    return [(1, 255), (255, 1), (256, 256), (257, 40000), (257, 16384), (16385, 257), (0, 16385), (0, 0), (0, 257)]


@functools.lru_cache(maxsize=None)
def selection_cases():
    cases = []
    # the radius is strict in the search (d2 < r^2) and not in the gate (sqrt(d2) > r drops): key 0 is
    # exactly 5 m from the last key pose
    b = [(3, 4, 0), (20, 0, 0), (0, 0, 0)]
    cases.append(_case("boundary_short_window", 1, b, dict(search_radius=5.0, recent_window=0.5), 4.1, times=[0, 2, 4],
                       shape=dict(n_frames=2, hits=[2], keys=[2, 2], dropped=[])))
    cases.append(_case("boundary_long_window", 1, b, dict(search_radius=5.0, recent_window=100.0), 4.1, times=[0, 2, 4],
                       shape=dict(n_frames=4, hits=[2], keys=[2, 2, 1, 0], dropped=[2])))
    cases.append(_case("zero_radius", 2, [(1, 1, 1), (0, 0, 0), (1, 1, 1)], dict(search_radius=0.0, recent_window=100.0), 3.0,
                       shape=dict(n_frames=3, hits=[], keys=[2, 1, 0], dropped=[1])))
    # four poses in the pose voxel [0, 2)^3 and the last one 10 m away: the merged record carries the
    # centroid and the mean index 1.5, which (int) truncates to key 1
    m = [(0.25, 0.5, 0.25), (1.5, 0.25, 0.5), (0.5, 1.75, 1.0), (1.75, 1.0, 1.25), (10.5, 0.5, 0.5)]
    cases.append(_case("merged_poses", 3, m, dict(search_radius=15.0, recent_window=-1.0), 10.0,
                       shape=dict(n_frames=2, hits=[4, 3, 1, 2, 0], keys=[1, 4], dropped=[], sources=["ds", "ds"])))
    # times are not monotone: walking back, key 2 (time 1) fails the window and stops the scan with the
    # newer key 1 behind it.  Key 1 is exactly on the radius: the search misses it, the gate would keep it.
    w = [(9, 0, 0), (3, 4, 0), (1.5, -2.5, 0), (-2.5, 1, 0), (0, 0, 0)]
    cases.append(_case("window_stop", 4, w, dict(search_radius=5.0, recent_window=3.0), 10.5, times=[0, 9, 1, 9.5, 10],
                       shape=dict(n_frames=5, hits=[4, 3, 2], keys=[2, 3, 4, 4, 3], dropped=[], absent=[1])))
    cases.append(_case("window_zero", 4, w, dict(search_radius=5.0, recent_window=0.0), 10.5, times=[0, 9, 1, 9.5, 10],
                       shape=dict(n_frames=3, hits=[4, 3, 2], keys=[2, 3, 4], dropped=[])))
    # loop mode takes submap_size + 1 frames (`<=`, :863); N = 6
    lp = [(1.5 * k, 0.5 * (k % 2), 0.1 * k) for k in range(6)]
    for sub, nf in ((0, 1), (4, 5), (5, 6), (9, 6)):
        cases.append(_case("loop_submap_%d" % sub, 5, lp, dict(loop_closure=1, submap_size=sub), 6.0,
                           shape=dict(n_frames=nf, keys=list(range(5, 5 - nf, -1)), dropped=[])))
    # ... and extractCloud's gate still applies to them
    cases.append(_case("loop_gated", 5, lp, dict(loop_closure=1, submap_size=9, search_radius=4.0), 6.0,
                       shape=dict(n_frames=6, keys=[5, 4, 3, 2, 1, 0], dropped=[3, 4, 5])))
    # segment sizes around the 256-lane block, the 64-block grid (16384 points) and beyond
    sz = _segment_sizes()
    sxyz = [(0.7 * k, -0.4 * k, 0.05 * k) for k in range(len(sz))]
    seg = _case("segment_sizes", 6, sxyz, dict(loop_closure=1, submap_size=100), 9.0, sizes=sz,
                shape=dict(n_frames=9, keys=list(range(8, -1, -1)), dropped=[], large=True))
    rng = np.random.default_rng(60)  # the big clouds spread over a 40 m x 40 m x 4 m box
    for k, (a, b_) in enumerate(sz):
        seg["corners"][k] = cloud(rng, a, (20.0, 20.0, 2.0))
        seg["surfs"][k] = cloud(rng, b_, (20.0, 20.0, 2.0))
    cases.append(seg)
    # the last three keyframes only: every corner segment is empty, so the corner launch has no work
    # while the surf launch has, and the corner map is empty
    cases.append(dict(seg, name="segment_sizes_no_corner", kp=dict(loop_closure=1, submap_size=2),
                      shape=dict(n_frames=3, keys=[8, 7, 6], dropped=[], corner_points=0)))
    return cases


@functools.lru_cache(maxsize=None)
def many_segments_case():
    """65537 keyframes of one corner and one surf point inside a 20 m box, all selected (loop mode)."""
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-10.0, 10.0, (N_MANY, 3)).astype(np.float32)
    poses = key_poses(xyz, None, rng)
    cpool, spool = cloud(rng, N_MANY), cloud(rng, N_MANY)
    return dict(name="many_segments", poses=poses, corners=[cpool[k:k + 1] for k in range(N_MANY)],
                surfs=[spool[k:k + 1] for k in range(N_MANY)], kp=dict(loop_closure=1, submap_size=N_MANY - 1), stamp=0.0,
                shape=dict(n_frames=N_MANY, dropped=[]))


def kparams(case):
    return keyframe_params(**case["kp"])


@functools.lru_cache(maxsize=None)
def loop_inputs():
    """The mapping loop: test_keyframes.make_keyframes(16) (seed 7, step 1.5), and for step k = 1..15 the
    extraction stamp, the next scan (at the trajectory's pose k + 1), its features and the perturbed
    guess test_keyframes.py registers from."""
    import pyoracle as O
    from feature_base_pointcloud_registration_amd import synth
    from test_keyframes import make_keyframes
    P, poses, corners, surfs, gt_last = make_keyframes(LOOP_N)
    traj = synth.trajectory(7, LOOP_N + 1, step=1.5)
    assert np.array_equal(np.asarray(traj[LOOP_N], np.float32), np.asarray(gt_last, np.float32))
    steps = []
    for k in range(1, LOOP_N):
        gt = traj[k + 1]
        scan = synth.scan(gt, 16, 1800, seed=999)
        f = O.Stream(P).features(scan)
        guess = np.asarray(gt, np.float32).copy()
        guess[:3] += np.float32([0.01, -0.01, 0.02])
        guess[3:] += np.float32([0.2, -0.15, 0.05])
        steps.append(dict(k=k, stamp=float(poses["time"][k]) + 0.5, gt=np.asarray(gt, np.float32), scan=scan,
                          corner=f["corner"], surf=f["surf"], guess=guess))
    moved = poses.copy()  # correctPoses after a loop closure: every key pose moves
    moved["x"] += (0.05 + 0.01 * np.arange(LOOP_N)).astype(np.float32)
    moved["y"] -= np.float32(0.03)
    moved["yaw"] += np.float32(0.002)
    moved["pitch"] -= np.float32(0.001)
    return dict(poses=poses, corners=corners, surfs=surfs, steps=steps, moved=moved, kp=dict(LOOP_KP),
                shrunk_kp=dict(LOOP_KP, search_radius=1.0))
