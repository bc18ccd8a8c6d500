"""Pose scoring restated (include/fbr.h "pose scoring"): a NumPy float32 brute force in the device's
operation order, the lattice generator and the selection order.  TEST INFRASTRUCTURE ONLY; NumPy and
tests/knn_model.py alone, but for the shared references at the end, which take the installed map's
order from the CPU oracle's VoxelGrid (tests/test_score_model.py checks this file on the CPU, tests/test_pose_score.py
compares the device with it key for key).

Because the distances are the same float32 arithmetic (knn_model.dist2) and a correspondence is the
smallest 64-bit key (bits(d2) << 32) | map index, no query is ambiguous: the device has to return
the same keys, hence the same counts, and sums that differ only by the order of the double additions.
"""
import functools

import numpy as np

import knn_model as K

F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SEARCH_MAX = 1 << 20
SCORE = np.dtype([("n", np.int32, 2), ("n_in", np.int32, 2), ("sum_d2", np.float64, 2), ("fitness", np.float64)])


def gate2(gate):
    g = F(gate)
    return F(g * g)


def nn_keys(map_xyz, q, g2, box=None, chunk=128):
    """uint64 [len(q)]: the smallest (bits(d2) << 32) | map index over the map points inside the
    inclusive box (None: all of them), kept where d2 < g2; NONE elsewhere and for a non-finite q."""
    m = np.ascontiguousarray(map_xyz, F).reshape(-1, 3)
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    idx = np.arange(len(m), dtype=np.uint64)
    if box is not None:
        keep = np.all((m >= np.asarray(box[0], F)) & (m <= np.asarray(box[1], F)), axis=1)  # pcl::CropBox, inclusive
        m, idx = m[keep], idx[keep]
    out = np.full(len(q), NONE, np.uint64)
    if len(m) == 0:
        return out
    empty = np.uint64(int(np.asarray(g2, F).view(np.uint32))) << np.uint64(32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, len(q), chunk):
            qq = q[r0:r0 + chunk]
            d = K.dist2(qq, m)
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]
            best = key.min(axis=1)
            ok = np.isfinite(qq).all(axis=1) & (best < empty)
            out[r0:r0 + chunk] = np.where(ok, best, NONE)
    return out


def key_d2(keys):
    """The float32 d2 of each key (0 where there is none)."""
    k = np.asarray(keys, np.uint64)
    return np.where(k == NONE, np.uint64(0), k >> np.uint64(32)).astype(np.uint32).view(F)


def record(n_corner, keys, g2):
    """The fbr_pose_score record of one pose from its keys (corner points first)."""
    r = np.zeros((), SCORE)
    n = (n_corner, len(keys) - n_corner)
    tot = 0.0
    for k, sl in enumerate((slice(0, n_corner), slice(n_corner, None))):
        kk = keys[sl]
        inl = kk != NONE
        r["n"][k], r["n_in"][k] = n[k], int(inl.sum())
        r["sum_d2"][k] = float(key_d2(kk[inl]).astype(np.float64).sum())
    n_total, n_in = int(sum(n)), int(r["n_in"].sum())
    tot = (r["sum_d2"][0] + r["sum_d2"][1]) + float(n_total - n_in) * float(g2)
    r["fitness"] = tot / n_total if n_total else np.finfo(np.float64).max
    return r


def score(corner_map, surf_map, corner, surf, T, crop_half, gate=1.0, use_crop=True, pre=None):
    """(record, keys) of the scan-frame clouds (n, 3) at the pose whose affine is T (rows 0-2 used,
    float32).  pre: a function (map, queries) -> ascending indices of a superset of the map points
    within 1 m of a query (knn_model.near, for large maps); the keys carry the full map's indices
    either way."""
    T = np.asarray(T, F).reshape(-1, 4)[:3]
    g2 = gate2(gate)
    box = None
    if use_crop:
        h = np.asarray(crop_half, F)
        box = ((-h) + T[:, 3], h + T[:, 3])
    keys = []
    for m, p in ((corner_map, corner), (surf_map, surf)):
        m = np.ascontiguousarray(m, F).reshape(-1, 3)
        q = K.associate(T[:, :4].reshape(12), p) if len(p) else np.zeros((0, 3), F)
        if pre is not None and len(q):
            # queries in spatial runs of 256 (8 m cells, then x), each against the map points near it
            k = np.full(len(q), NONE, np.uint64)
            fin = np.flatnonzero(np.isfinite(q).all(axis=1))
            cell = np.floor(q[fin].astype(np.float64) / 8.0)
            fin = fin[np.lexsort((q[fin][:, 0], cell[:, 0], cell[:, 1], cell[:, 2]))]
            for r0 in range(0, len(fin), 256):
                run = fin[r0:r0 + 256]
                sub = pre(m, q[run])
                kk = nn_keys(m[sub], q[run], g2, box)
                hit = kk != NONE
                kk[hit] = (kk[hit] & ~np.uint64(0xFFFFFFFF)) | sub[(kk[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)].astype(np.uint64)
                k[run] = kk
        else:
            k = nn_keys(m, q, g2, box)
        keys.append(k)
    keys = np.concatenate(keys)
    return record(len(corner), keys, g2), keys


# ------------------------------------------------------------------------------------ the lattice
def axis_offsets(half, step):
    half, step = F(half), F(step)
    if not (np.isfinite(half) and np.isfinite(step) and half >= 0 and step >= 0):
        raise ValueError("half and step are finite and non-negative")
    if half == 0 or step == 0:
        return np.zeros(1, F)
    k = int(np.floor(half / step))  # float32 division
    if k > SEARCH_MAX:
        raise ValueError("more than 2^20 hypotheses")
    return (np.arange(-k, k + 1).astype(F) * step).astype(F)


def lattice(seeds, half, step):
    """The hypotheses of fbr_pose_search, float32 [n, 6]: seed-major, then yaw, z, y, x (x fastest),
    every axis ascending; offsets i * step for |i| <= floor(half / step), added in float32."""
    seeds = np.asarray(seeds, F).reshape(-1, 6)
    ox, oy, oz, oyaw = (axis_offsets(h, s) for h, s in zip(half, step))
    per = len(ox) * len(oy) * len(oz) * len(oyaw)
    if per * len(seeds) > SEARCH_MAX:
        raise ValueError("more than 2^20 hypotheses")
    W, Zz, Y, X = np.meshgrid(oyaw, oz, oy, ox, indexing="ij")
    out = np.zeros((len(seeds), per, 6), F)
    out[:, :, :2] = seeds[:, None, :2]
    for col, off in ((2, W), (3, X), (4, Y), (5, Zz)):
        out[:, :, col] = seeds[:, None, col] + off.ravel()[None, :]
    return out.reshape(-1, 6)


def order(fitness, top_k):
    """Indices of the top_k smallest by (fitness, index)."""
    return np.argsort(np.asarray(fitness, np.float64), kind="stable")[:max(int(top_k), 0)]


# ------------------------------------------------------------------------------------ shared references
STRUCT_LATTICE = ((0.5, 0.5, 0.0, 0.1), (0.25, 0.25, 0.0, 0.05))  # 5 x 5 x 1 x 5 = 125 poses around gt
STRUCT_CROP_HALF = (30.0, 30.0, 10.0)                            # fbr_params' default box


def affine32(pose):
    """Rows 0-2 of pcl::getTransformation in float32 with the library's host sinf / cosf
    (fbr_affine_from_pose: no GPU needed)."""
    from feature_base_pointcloud_registration_amd import api
    return api.affine_from_pose(np.asarray(pose, F))[:3]


@functools.lru_cache(maxsize=None)
def structured_reference():
    """knn_model.structured_case() scored at the 125 poses of STRUCT_LATTICE around its gt (gate 1 m,
    registration's box at STRUCT_CROP_HALF): dict(case, poses, records, keys, order), computed once."""
    import pyoracle as O
    s = dict(K.structured_case())
    # the map as fbr_set_map installs it: the start-up VoxelGrid keeps every point (one per voxel)
    # but puts them in voxel order, and a key carries the installed map's index
    s["corner_map"], s["surf_map"] = O.voxel_grid(s["corner_map"], K.LEAF_C), O.voxel_grid(s["surf_map"], K.LEAF_S)
    poses = lattice(s["gt"][None], *STRUCT_LATTICE)
    cm, sm, c, p = (K.xyz_of(s[k]) for k in ("corner_map", "surf_map", "corner", "surf"))
    recs, keys = [], []
    for pose in poses:
        r, k = score(cm, sm, c, p, affine32(pose), STRUCT_CROP_HALF)
        recs.append(r)
        keys.append(k)
    recs = np.array(recs, SCORE)
    return dict(case=s, poses=poses, records=recs, keys=np.array(keys), order=order(recs["fitness"], len(poses)))


# The C1 relocalisation (tests/sc_fixtures.py): seeds off the truth by (x m, y m, yaw rad), and the
# lattice searched around them, 13 x 13 x 17 = 2,873 poses that do not contain the truth
SEED_OFFSETS = {1: (2.2, -1.3, 0.63), 3: (-2.7, 1.2, -0.74)}
RELOC_LATTICE = ((3.0, 3.0, 0.0, 0.8), (0.5, 0.5, 0.0, 0.1))


def reloc_seed(q):
    import sc_fixtures as SF
    dx, dy, dyaw = SEED_OFFSETS[q]
    return (SF.reloc()["queries"][q]["gt"] + np.array([0, 0, dyaw, dx, dy, 0])).astype(F)


@functools.lru_cache(maxsize=None)
def reloc_seed_oracle(q):
    """The CPU oracle's registration of C1 query q from its coarse seed: (pose, stats)."""
    import sc_fixtures as SF
    Q = SF.reloc()["queries"][q]
    pose, st, _ = SF._oracle_map().register(Q["feat"]["corner"], Q["feat"]["surf"], reloc_seed(q))
    return pose, st
