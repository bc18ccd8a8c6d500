"""Fixtures shared by tests/test_sc_model.py (CPU) and tests/test_scan_context.py (GPU): the loop
fixture of tests/test_loop_closure.py with the last key pose drifted out of the radius search, and
the relocalisation grid.  TEST INFRASTRUCTURE ONLY.  Everything is computed once and never changed.
"""
import functools

import numpy as np

import loop_model as LM
import pyoracle as O
import sc_model as SM
import test_loop_closure as TL
from feature_base_pointcloud_registration_amd import synth
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, default_params, sc_params

DRIFT_X = 40.0   # added to keyframe 19's stored x: far outside historyKeyframeSearchRadius (15 m)

# What the CPU model measured on the two fixtures (tests/test_sc_model.py asserts that it still
# does); the GPU tests take their ground-truth bounds from these, not from the device.
MODEL_LOOP_ERR = (0.0078, 8.4e-5)     # pose_corrected of the re-anchored loop closure: m, rad
RELOC_BOUND = (0.05, 0.01)            # oracle registration from the hypothesis: m, rad


def descriptors(corners, surfs, sp, exact=True):
    """Model descriptors of keyframe clouds; exact: the probe's (= the device's) cells."""
    return [SM.keyframe_descriptor(c, s, sp, SM.probe_cells if exact else None) for c, s in zip(corners, surfs)]


@functools.lru_cache(maxsize=None)
def loop_drift():
    """test_loop_closure's out-and-back run with keyframe 19's stored x + 40 m.  Returns a dict: P,
    poses (drifted), corners, surfs, lp, sp, descs, detect (the model's), anchored (poses with
    keyframe 19 at the hypothesis), model (loop_model.perform on them)."""
    P, poses0, corners, surfs, lp, _ = TL.fixture()
    poses = poses0.copy()
    poses["x"][TL.N_KF - 1] += np.float32(DRIFT_X)
    sp = sc_params()
    descs = descriptors(corners, surfs, sp)
    found, best = SM.detect(poses, descs, TL.STAMP, lp, sp)
    guess = SM.pose_guess(LM.pose_of(poses[best[0]]), best[1], sp.n_sector)
    anchored = poses.copy()
    for name, v in zip(("roll", "pitch", "yaw", "x", "y", "z"), guess):
        anchored[name][TL.N_KF - 1] = v
    model = LM.perform(P, anchored, corners, surfs, TL.STAMP, lp)
    return dict(P=P, poses=poses, corners=corners, surfs=surfs, lp=lp, sp=sp, descs=descs, found=found, best=best,
                guess=guess, anchored=anchored, model=model)


# ---- relocalisation: 12 keyframes on an 8 m grid, yaw 0.3 i - 0.2 j, z = 1.8 ------------------------
GRID = [(i, j) for j in range(3) for i in range(4)]
# (keyframe, offset x, offset y, yaw turn): 0.5 .. 1.4 m off the keyframe, turned by 0.47 .. 3.0 rad
QUERIES = [(0, 0.4, 0.3, 0.47), (5, -0.7, 0.6, 1.3), (6, 0.9, -0.8, 2.1), (10, -1.0, -0.98, 3.0), (3, 0.3, -1.1, 0.9)]


def grid_pose(k):
    i, j = GRID[k]
    return np.array([0.0, 0.0, 0.3 * i - 0.2 * j, 8.0 * (i - 1.5), 8.0 * (j - 1.0), 1.8])


def query_pose(q):
    k, dx, dy, dyaw = QUERIES[q]
    p = grid_pose(k)
    p[2] += dyaw
    p[3] += dx
    p[4] += dy
    return p


def _features(P, gt, seed):
    f = O.Stream(P).features(synth.scan(gt, 16, 1800, seed=seed))
    return f, O.voxel_grid(f["corner"], P.mapping_corner_leaf_size), O.voxel_grid(f["surf"], P.mapping_surf_leaf_size)


@functools.lru_cache(maxsize=None)
def reloc():
    """dict: P, poses (KEYPOSE), corners, surfs (mapping-leaf DS, lidar frame), sp, descs, map (the C1
    prior map clouds), queries = [dict(gt, scan, feat, corner_ds, surf_ds, desc, rank, guess)]."""
    P = default_params(16, 1800)
    sp = sc_params()
    poses = np.zeros(len(GRID), KEYPOSE)
    corners, surfs = [], []
    for k in range(len(GRID)):
        gt = grid_pose(k)
        _, c, s = _features(P, gt, 300 + k)
        corners.append(c)
        surfs.append(s)
        poses[k] = (gt[3], gt[4], gt[5], k, gt[0], gt[1], gt[2], 0.0, 2.0 * k)
    descs = descriptors(corners, surfs, sp)
    queries = []
    for q in range(len(QUERIES)):
        gt = query_pose(q)
        scan = synth.scan(gt, 16, 1800, seed=400 + q)
        f = O.Stream(P).features(scan)
        c = O.voxel_grid(f["corner"], P.mapping_corner_leaf_size)
        s = O.voxel_grid(f["surf"], P.mapping_surf_leaf_size)
        d = SM.keyframe_descriptor(c, s, sp, SM.probe_cells)
        r = SM.rank(d, descs)
        guess = SM.pose_guess(LM.pose_of(poses[r[0][0]]), r[0][1], sp.n_sector)
        queries.append(dict(gt=gt, scan=scan, feat=f, corner_ds=c, surf_ds=s, desc=d, rank=r, guess=guess))
    return dict(P=P, poses=poses, corners=corners, surfs=surfs, sp=sp, descs=descs, map=synth.config_map("C1"),
                queries=queries)


@functools.lru_cache(maxsize=None)
def reloc_oracle(q, from_identity=False):
    """The CPU oracle's registration of query q against the C1 map from the model's hypothesis (or
    from the identity guess): (pose, stats)."""
    R = reloc()
    omap = _oracle_map()
    Q = R["queries"][q]
    guess = np.zeros(6, np.float32) if from_identity else Q["guess"]
    pose, st, _ = omap.register(Q["feat"]["corner"], Q["feat"]["surf"], guess)
    return pose, st


@functools.lru_cache(maxsize=None)
def _oracle_map():
    R = reloc()
    return O.Map(R["P"], *R["map"])


def pose_err(p, gt):
    """(translation error m, largest angle error rad)."""
    p, gt = np.asarray(p, np.float64), np.asarray(gt, np.float64)
    return float(np.linalg.norm(p[3:] - gt[3:])), float(np.abs(np.angle(np.exp(1j * (p[:3] - gt[:3])))).max())


# ---- synthetic descriptors, written through keyframes of one point per non-zero cell ---------------
def random_descriptor(rng, sp, fill=1.0):
    """Cell values on multiples of 1/8 in [0.125, 4] (exact in float32, also as z = v - lidar_height
    for the default height 2), a fraction `fill` of the cells non-zero."""
    d = (rng.integers(1, 33, (sp.n_ring, sp.n_sector)) / 8.0).astype(np.float32)
    if fill < 1.0:
        d[rng.random(d.shape) >= fill] = 0.0
    return d


def cloud_of(D, sp):
    """One point at the centre of every non-zero cell of D, at the height that gives the cell's value."""
    from feature_base_pointcloud_registration_amd.fbr_types import POINT_XYZI
    ring, sector = np.nonzero(D)
    r = (ring + 0.5) / sp.n_ring * float(np.float32(sp.max_radius))
    th = (sector + 0.5) / sp.n_sector * 2.0 * np.pi
    c = np.zeros(len(ring), POINT_XYZI)
    c["x"], c["y"] = r * np.cos(th), r * np.sin(th)
    c["z"] = D[ring, sector] - np.float32(sp.lidar_height)
    return c


def perturbed(rng, D, frac, sp):
    """D with a fraction `frac` of its cells drawn anew."""
    out = D.copy()
    m = rng.random(D.shape) < frac
    out[m] = random_descriptor(rng, sp)[m]
    return out


@functools.lru_cache(maxsize=None)
def search_cases():
    """name -> dict(sp, query, cands, ks): the query descriptor, the candidates' descriptors in
    keyframe order and the k values asked for.  The candidates are rotated copies of the query with
    a growing share of their cells redrawn, so the distances spread over [0, ~0.25]."""
    rng = np.random.default_rng(77)
    cases = {}

    def spread(sp, n):
        q = random_descriptor(rng, sp)
        cands = [np.roll(perturbed(rng, q, (i + 1.0) / (n + 1.0), sp), int(rng.integers(0, sp.n_sector)), axis=1)
                 for i in rng.permutation(n)]
        return q, cands

    sp = sc_params()
    q, c = spread(sp, 1)
    cases["n0"] = dict(sp=sp, query=q, cands=[], ks=[4])
    cases["n1"] = dict(sp=sp, query=q, cands=c, ks=[1, 4])
    q, c = spread(sp, 65)
    cases["n65"] = dict(sp=sp, query=q, cands=c, ks=[1, 16])
    small = sc_params(n_ring=3, n_sector=12)
    q, c = spread(small, 257)
    cases["n257_3x12"] = dict(sp=small, query=q, cands=c, ks=[1, 16])
    big = sc_params(n_ring=32, n_sector=64)
    q, c = spread(big, 5)
    cases["n5_32x64"] = dict(sp=big, query=q, cands=c, ks=[8])
    tiny = sc_params(n_ring=1, n_sector=2)
    cases["n3_1x2"] = dict(sp=tiny, query=np.float32([[1.0, 2.0]]),
                           cands=[np.float32([[2.0, 1.0]]), np.float32([[1.0, 2.0]]), np.float32([[0.0, 3.0]])], ks=[3])
    # the query rotated by 0, 1 and n_sector - 1 (equal distances: the lower index first), a candidate
    # twice (keyframes 3 and 5), an all-zero candidate (distance 1.0), candidates with empty columns
    q = random_descriptor(rng, sp)
    a = perturbed(rng, q, 0.3, sp)
    holes = perturbed(rng, q, 0.2, sp)
    holes[:, [0, 7, 8, 31, 59]] = 0.0
    holes2 = np.roll(holes, 5, axis=1)
    cases["edges"] = dict(sp=sp, query=q,
                          cands=[np.roll(q, 59, axis=1), np.roll(q, 0, axis=1), np.roll(q, 1, axis=1), a, holes, a.copy(),
                                 np.zeros_like(q), holes2], ks=[8])
    # a query with empty columns of its own against the same candidates
    qh = q.copy()
    qh[:, [3, 7, 40, 41, 42]] = 0.0
    cases["edges_query_holes"] = dict(sp=sp, query=qh, cands=cases["edges"]["cands"], ks=[8])
    # column period n_sector / 2: shifts s and s + 30 tie exactly, the lowest wins
    half = random_descriptor(rng, sc_params(n_sector=30))
    qp = np.concatenate([half, half], axis=1)
    # (with a periodic query only a periodic candidate is decidable: for any other one the two shifts
    # sum the same terms in another order)
    half2 = perturbed(rng, half, 0.1, sc_params(n_sector=30))
    cases["period"] = dict(sp=sp, query=qp, cands=[np.roll(qp, 37, axis=1),
                                                   np.roll(np.concatenate([half2, half2], axis=1), 33, axis=1)], ks=[2])
    return cases


def search_poses(n):
    """Stored key poses of the search cases' keyframes: roll and pitch 0.01, everything else varied."""
    poses = np.zeros(n, KEYPOSE)
    for k in range(n):
        poses[k] = (3.0 * k - 20.0, 0.7 * k, 1.8 + 0.01 * k, k, 0.01, 0.01, 0.37 * k - 3.0, 0.0, 2.0 * k)
    return poses
