"""NumPy restatement of the place-recognition contract of include/fbr.h (scan-context descriptors,
the exhaustive shift search, ranking, the pose hypothesis).  TEST INFRASTRUCTURE ONLY.

Bins in float64 from the float32 coordinates, cell values in float32 (they are compared exactly),
the distance sums in float64 in the header's order.  A float64 bin equals the device's float32 bin
except within rounding of a bin edge: tests on real clouds pass the probe's cells (tests/native/
sc_probe.cpp, the device's own function, checked against bins() away from the edges) as `cells`.
"""
import ctypes
import functools

import numpy as np

import loop_model as LM
import pyoracle as O

F32 = np.float32
TWO_PI = 2.0 * np.pi


def xyz(cloud):
    """(n, 3) float32 of a POINT_XYZI array (or of an (n, 3) array)."""
    if getattr(cloud, "dtype", None) is not None and cloud.dtype.names:
        return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F32)
    return np.asarray(cloud, F32).reshape(-1, 3)


def polar(pts):
    """(r / max_radius-free range, theta in [0, 2 pi)) in float64."""
    p = xyz(pts).astype(np.float64)
    r = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
    th = np.arctan2(p[:, 1], p[:, 0])
    th = np.where(th < 0, th + TWO_PI, th)
    return r, th


def bins(pts, sp):
    """cell = ring * n_sector + sector per point, -1 for a dropped one (float64 arithmetic)."""
    p = xyz(pts)
    r, th = polar(p)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(p).all(1) & (r < float(F32(sp.max_radius)))
        ring = np.minimum(sp.n_ring - 1, np.floor(np.where(keep, r, 0.0) / float(F32(sp.max_radius)) * sp.n_ring))
        sector = np.minimum(sp.n_sector - 1, np.floor(np.where(keep, th, 0.0) / TWO_PI * sp.n_sector))
    cell = (ring * sp.n_sector + sector).astype(np.int64)
    return np.where(keep, cell, -1).astype(np.int32)


def edge_margin(pts, sp):
    """Per point: the distance to the nearest ring / sector edge in units of a bin (min of the two)."""
    r, th = polar(pts)
    fr = r / float(F32(sp.max_radius)) * sp.n_ring
    fs = th / TWO_PI * sp.n_sector
    m = lambda f: np.minimum(f - np.floor(f), np.ceil(f) - f)
    with np.errstate(invalid="ignore"):  # (a non-finite point has no margin: NaN compares false)
        return np.minimum(m(fr), m(fs))  # floor == ceil on an exact edge gives 0, as it should


def descriptor(pts, sp, cells=None):
    """D[n_ring, n_sector] float32: per cell the maximum of max(z + lidar_height, 0) in float32."""
    p = xyz(pts)
    cell = bins(p, sp) if cells is None else np.asarray(cells)
    with np.errstate(all="ignore"):
        t = (p[:, 2] + F32(sp.lidar_height)).astype(F32)
    v = np.where(t > 0, t, F32(0)).astype(F32)
    d = np.zeros(sp.n_ring * sp.n_sector, F32)
    ok = cell >= 0
    np.maximum.at(d, cell[ok], v[ok])
    return d.reshape(sp.n_ring, sp.n_sector)


def column_norms(D):
    """sqrt of the double sum of squares, rings ascending."""
    D = np.asarray(D, F32).astype(np.float64)
    s = np.zeros(D.shape[1])
    for r in range(D.shape[0]):
        s = s + D[r] * D[r]
    return np.sqrt(s)


def distances(Q, C):
    """d(s) for every shift s, float64 [n_sector]."""
    Q, C = np.asarray(Q, F32).astype(np.float64), np.asarray(C, F32).astype(np.float64)
    R, S = Q.shape
    qn, cn = column_norms(Q), column_norms(C)
    idx = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S   # [shift, column] -> candidate column
    dot = np.zeros((S, S))
    for r in range(R):
        dot = dot + Q[r][None, :] * C[r][idx]
    ok = (qn[None, :] > 0) & (cn[idx] > 0)
    with np.errstate(all="ignore"):
        cos = np.where(ok, dot / (qn[None, :] * cn[idx]), 0.0)
    total = np.zeros(S)
    for c in range(S):   # columns ascending (a column that does not count adds an exact 0)
        total = total + cos[:, c]
    n_eff = ok.sum(1)
    with np.errstate(all="ignore"):
        return np.where(n_eff > 0, 1.0 - total / np.maximum(n_eff, 1), 1.0)


def match(Q, C):
    """(distance, shift): the minimum over the shifts, ties to the lowest shift."""
    d = distances(Q, C)
    s = int(np.argmin(d))
    return float(d[s]), s


def rank(Q, candidates, k=None, eligible=None):
    """[(keyframe, shift, distance)] by (distance, keyframe index) ascending, the first k."""
    out = []
    for i, C in enumerate(candidates):
        if eligible is not None and not eligible[i]:
            continue
        d, s = match(Q, C)
        out.append((i, s, d))
    out.sort(key=lambda t: (t[2], t[0]))
    return out if k is None else out[:k]


def pose_guess(pose6, shift, n_sector):
    """The hypothesis of a match: float32 [roll, pitch, yaw, x, y, z] of (stored pose) * Rz(delta)."""
    delta = F32(np.float64(shift) * TWO_PI / np.float64(n_sector))
    turn = np.array([0, 0, delta, 0, 0, 0], F32)
    return O.pose_from_affine(LM.compose(O.affine_from_pose(np.asarray(pose6, F32)), O.affine_from_pose(turn)))


def keyframe_descriptor(corner, surf, sp, cells_fn=None):
    pts = np.concatenate([xyz(corner), xyz(surf)])
    return descriptor(pts, sp, None if cells_fn is None else cells_fn(pts, sp))


def detect(poses, descs, stamp, lp, sp):
    """fbr_sc_detect_loop_closure: ((latest, closest) or None, best (keyframe, shift, distance) or None)."""
    n = len(poses)
    if n < 2:
        return None, None
    elig = [abs(float(poses["time"][i]) - stamp) > float(F32(lp.search_time_diff)) for i in range(n - 1)]
    r = rank(descs[n - 1], descs[:n - 1], 1, elig)
    if not r:
        return None, None
    best = r[0]
    return ((n - 1, best[0]) if best[2] < float(F32(sp.dist_threshold)) else None), best


# ---- the CPU probe of csrc/fbr_sc.h ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe():
    from conftest import build_probe
    L = build_probe("sc_probe")
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.probe_sc_cells.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp]
    L.probe_sc_descriptor.argtypes = [vp, i64, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp]
    L.probe_sc_distances.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    for f in (L.probe_sc_cells, L.probe_sc_descriptor, L.probe_sc_distances):
        f.restype = None
    return L


def probe_cells(pts, sp):
    p = np.ascontiguousarray(xyz(pts))
    out = np.zeros(max(len(p), 1), np.int32)
    probe().probe_sc_cells(p.ctypes.data, len(p), sp.n_ring, sp.n_sector, sp.max_radius, out.ctypes.data)
    return out[:len(p)]


def probe_descriptor(pts, sp):
    p = np.ascontiguousarray(xyz(pts))
    out = np.zeros((sp.n_ring, sp.n_sector), np.float32)
    probe().probe_sc_descriptor(p.ctypes.data, len(p), sp.n_ring, sp.n_sector, sp.max_radius, sp.lidar_height,
                                out.ctypes.data)
    return out


def probe_distances(Q, C):
    Q, C = np.ascontiguousarray(Q, F32), np.ascontiguousarray(C, F32)
    out = np.zeros(Q.shape[1], np.float64)
    probe().probe_sc_distances(Q.ctypes.data, C.ctypes.data, Q.shape[0], Q.shape[1], out.ctypes.data)
    return out
