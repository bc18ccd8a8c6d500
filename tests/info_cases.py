"""The worlds of the registration-information tests (NumPy only, fixed seeds).

tiny(): the tiny set of tests/test_gn_direct.py (60 corner queries: one item inside a single wave;
300 surf queries: a full item and one of 44 rows) on the structured world of tests/knn_model.py.

corridor(): a floor and two parallel walls along x, every map point on an exact plane of the 0.5 m
lattice, the wall-floor edges as the corner map (0.25 m apart).  Nothing in it says where along x
the sensor is, so the normal matrix has one eigenvalue near zero, along x.  end_wall=True closes
the corridor at x = 6 and observes x.  The scan is the world seen from `pose` (yaw 0 or pi / 2), a
few hundred points off the lattice with 5 mm of noise along each plane's normal.
"""
import numpy as np

import knn_model as K

F = np.float32
CORRIDOR_CROP = (50.0, 50.0, 50.0)  # the whole corridor lies inside registration's box


def tiny():
    from test_gn_direct import tiny_of
    return tiny_of(K.structured_case())


def corridor_map(end_wall=False):
    gx = np.arange(-12, 13) * 0.5
    gy = np.arange(-4, 5) * 0.5
    gz = np.arange(-3, 4) * 0.5
    floor = [(x, y, -1.5) for x in gx for y in gy]
    walls = [(x, s * 2.0, z) for x in gx for z in gz[1:] for s in (-1.0, 1.0)]
    end = [(6.0, y, z) for y in gy[1:-1] for z in gz[1:]] if end_wall else []
    surf = np.asarray(floor + walls + end, F)
    corner = np.asarray([(x, s * 2.0, -1.5) for x in np.arange(-24, 25) * 0.25 for s in (-1.0, 1.0)], F)
    rng = np.random.default_rng(11)
    return corner[rng.permutation(len(corner))], surf[rng.permutation(len(surf))]


def corridor(yaw=0.0, end_wall=False, centre=(0.0, 0.0, 0.0), seed=3):
    """{corner_map, surf_map (POINT_XYZI), corner, surf (scan frame, POINT_XYZI), pose (6,) float32}."""
    rng = np.random.default_rng(seed)
    cm, sm = corridor_map(end_wall)
    cx = float(centre[0])
    n = 100
    nz = lambda k: rng.normal(0.0, 0.005, k)  # noqa: E731
    fl = np.stack([rng.uniform(cx - 4.5, cx + 4.5, 120), rng.uniform(-1.3, 1.3, 120), -1.5 + nz(120)], 1)
    w = [np.stack([rng.uniform(cx - 4.5, cx + 4.5, n), s * 2.0 + nz(n), rng.uniform(-0.8, 1.3, n)], 1) for s in (-1.0, 1.0)]
    parts = [fl] + w
    if end_wall:
        parts.append(np.stack([6.0 + nz(200), rng.uniform(-1.3, 1.3, 200), rng.uniform(-0.8, 1.3, 200)], 1))
    edges = np.concatenate([np.stack([rng.uniform(cx - 4.5, cx + 4.5, 30), s * 2.0 + nz(30), -1.5 + nz(30)], 1) for s in (-1.0, 1.0)])
    pose = np.array([0.0, 0.0, yaw, centre[0], centre[1], centre[2]], F)
    T = K.pose_matrix64(pose)
    to_scan = lambda wpts: ((wpts - T[:, 3]) @ T[:, :3]).astype(F)  # noqa: E731
    return dict(corner_map=K.cloud(cm), surf_map=K.cloud(sm), corner=K.cloud(to_scan(edges)), surf=K.cloud(to_scan(np.vstack(parts))),
                pose=pose)


# ---- the search-edge cases (knn_model.lattice_cases) ----
# Queries whose acceptance hangs on a comparison within 4 float32 ulps of its threshold
# (info_model.ambiguous: the corner fit's eigenvalue gate, where the lattice gives covariance
# eigenvalues in the exact ratio 3, and one plane distance at 0.2), by case set and index into
# corner-then-surf.  They are taken out of the clouds; tests/test_reg_info_model.py asserts that this
# table is exactly what the model finds, so nothing else is dropped and nothing ambiguous stays.
LATTICE_DROPPED = {'grid_1': [198], 'ties_gate_crop_1': [7, 21], 'ties_gate_crop_2': [9], 'holes_0': [11, 16, 17, 21, 23],
                   'holes_1': [22], 'extent_pos_0': [19, 21, 22], 'extent_pos_1': [2, 23], 'extent_neg_0': [22],
                   'extent_neg_1': [12], 'extent_neg_2': [6, 8, 13, 14, 20, 22], 'shifted_box_0': [7, 9, 17, 26],
                   'far': [13, 23]}


def lattice_map():
    """The lattice map as fbr_set_map keeps it: the oracle's VoxelGrid at the mapping leaves (every
    lattice point has a voxel of its own; the filter decides the map-index order, which decides ties)."""
    import pyoracle as O
    lat = K.cloud(K.lattice_points())
    return lat, K.xyz_of(O.voxel_grid(lat, K.LEAF_C)), K.xyz_of(O.voxel_grid(lat, K.LEAF_S))


def lattice_clouds(case, dropped=True):
    """(corner, surf) of a lattice case as POINT_XYZI clouds, without the dropped queries."""
    nc = len(case["corner"])
    drop = LATTICE_DROPPED.get(case["name"], []) if dropped else []
    kc = np.setdiff1d(np.arange(nc), [i for i in drop if i < nc])
    ks = np.setdiff1d(np.arange(len(case["surf"])), [i - nc for i in drop if i >= nc])
    return case["corner"][kc].copy(), case["surf"][ks].copy()
