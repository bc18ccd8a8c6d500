"""NumPy float64 model of the motion path (include/fbr.h "Motion deskew", csrc/fbr_motion.h,
csrc/fbr_odom.cpp) and the test-scan generator skew_scan.

The model restates the reference, not the code under test: deskewPoint (imageProjection.cpp:545-580)
with findPosition's commented body live (:528-542), odomDeskewInfo (:395-491), updateInitialGuess
(mapOptmization.h:799-855), pcl::getTransformation / getTranslationAndEulerAngles and
tf::Matrix3x3::getRPY, all in float64.  Where bits are compared the tests use the host probe
(tests/native/motion_probe.cpp), which compiles the product header itself; the float32 restatement
here covers the two ratios, whose bits the probe's callers need.
"""
import numpy as np

import proj_model

POSITION, ROTATION = 1, 2


# ------------------------------------------------------------------------------- pose algebra
def rot_rpy(roll, pitch, yaw):
    A, B, C, D, E, F = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[A * C, A * D * F - B * E, B * F + A * D * E], [B * C, A * E + B * D * F, B * D * E - A * F],
                     [-D, C * F, C * E]])


def affine(p6):
    """pcl::getTransformation of {roll, pitch, yaw, x, y, z} as a 4x4."""
    p6 = np.asarray(p6, np.float64)
    T = np.eye(4)
    T[:3, :3] = rot_rpy(p6[0], p6[1], p6[2])
    T[:3, 3] = p6[3:]
    return T


def pose(T):
    """pcl::getTranslationAndEulerAngles into {roll, pitch, yaw, x, y, z}."""
    return np.array([np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0]),
                     T[0, 3], T[1, 3], T[2, 3]])


def quat_rpy(q):
    """tf::quaternionMsgToTF (normalised past QUATERNION_TOLERANCE) + Matrix3x3::getRPY; q = x, y, z, w."""
    q = np.asarray(q, np.float64)
    if abs(q @ q - 1) > 0.1:
        q = q / np.sqrt(q @ q)
    x, y, z, w = q
    s = 2.0 / (q @ q)
    m00, m10, m20 = 1 - s * (y * y + z * z), s * (x * y + w * z), s * (x * z - w * y)
    m21, m22 = s * (y * z + w * x), 1 - s * (x * x + y * y)
    if abs(m20) >= 1:
        return np.array([np.arctan2(m21, m22), np.pi / 2 if m20 < 0 else -np.pi / 2, 0.0])
    p = -np.arcsin(m20)
    return np.array([np.arctan2(m21 / np.cos(p), m22 / np.cos(p)), p, np.arctan2(m10 / np.cos(p), m00 / np.cos(p))])


# ------------------------------------------------------------------------------- deskewPoint
def ratio_field32(time, scan_period):
    """(float)((double)time / scan_period)"""
    return (np.asarray(time, np.float32).astype(np.float64) / np.float64(scan_period)).astype(np.float32)


def column_k(direction, col, col_first, W):
    return np.mod(direction * (np.asarray(col, np.int64) - int(col_first)), W)


def ratio_column32(direction, col, col_first, W):
    """(float)k / (float)W"""
    return column_k(direction, col, col_first, W).astype(np.float32) / np.float32(W)


def trans_final(incre, flags, ratio, rot=None):
    """getTransformation(pos, rot): pos = ratio * incre[3:] with POSITION; rot the given IMU angles,
    else ratio * incre[:3] with ROTATION, else 0."""
    incre = np.asarray(incre, np.float64)
    pos = ratio * incre[3:] if flags & POSITION else np.zeros(3)
    if rot is None:
        rot = ratio * incre[:3] if flags & ROTATION else np.zeros(3)
    return affine(np.concatenate([rot, pos]))


def deskew(incre, flags, ratio_first, ratio, xyz, rot_first=None, rot=None):
    """transBt * point for every point: transStartInverse = transFinal(first point)^-1."""
    xyz = np.asarray(xyz, np.float64)
    ratio = np.broadcast_to(np.asarray(ratio, np.float64), xyz.shape[:1])
    S = np.linalg.inv(trans_final(incre, flags, float(ratio_first), rot_first))
    out = np.empty_like(xyz)
    for i in range(len(xyz)):
        T = S @ trans_final(incre, flags, float(ratio[i]), None if rot is None else rot[i])
        out[i] = T[:3, :3] @ xyz[i] + T[:3, 3]
    return out


# ------------------------------------------------------------------------------- odomDeskewInfo
def odom_deskew_info(q, cur, nxt):
    """dict(odom_available, odom_deskew_flag, initial_guess, reset_id, incre, n_pop, start, end):
    start / end are the indices of the samples taken (None where the function returned before)."""
    out = dict(odom_available=0, odom_deskew_flag=0, initial_guess=np.zeros(6), reset_id=0, incre=np.zeros(6),
               n_pop=0, start=None, end=None)
    n = len(q)
    b = 0
    while b < n and q["stamp"][b] < cur - 0.01:
        b += 1
    out["n_pop"] = b
    if b == n or q["stamp"][b] > cur:
        return out

    def first_at(t):
        for i in range(b, n):
            if q["stamp"][i] >= t:
                return i
        return n - 1  # the loop leaves the last sample

    i0 = first_at(cur)
    rpy0 = quat_rpy(q["orientation"][i0])
    out.update(start=i0, odom_available=1, reset_id=int(np.round(q["covariance0"][i0])),
               initial_guess=np.concatenate([rpy0, q["position"][i0]]))
    if q["stamp"][n - 1] < nxt:
        return out
    i1 = first_at(nxt)
    out["end"] = i1
    if int(np.round(q["covariance0"][i0])) != int(np.round(q["covariance0"][i1])):
        return out
    A = affine(np.concatenate([rpy0, q["position"][i0]]))
    B = affine(np.concatenate([quat_rpy(q["orientation"][i1]), q["position"][i1]]))
    out.update(incre=pose(np.linalg.inv(A) @ B), odom_deskew_flag=1)
    return out


def motion_from_poses(prev, cur, dt, scan_period, dt_next):
    step = pose(np.linalg.inv(affine(prev)) @ affine(cur))
    return step * (scan_period / dt), pose(affine(cur) @ affine(step * (dt_next / dt)))


class GuessModel:
    """updateInitialGuess with its static lastImuTransformation."""

    def __init__(self, reset_id=0):
        self.reset_id = reset_id
        self.last = np.eye(4)

    def update(self, odom, imu_rpy, imu_available, have_keyframes, use_imu_heading, tr):
        tr = np.array(tr, np.float64)
        back = affine([imu_rpy[0], imu_rpy[1], imu_rpy[2], 0, 0, 0])
        if not have_keyframes:
            tr[:3] = imu_rpy
            if not use_imu_heading:
                tr[2] = 0
            self.last = back
            return tr
        if odom is not None and odom["odom_available"] and odom["reset_id"] == self.reset_id:
            tr[:] = odom["initial_guess"]
            self.last = back
            return tr
        if imu_available:
            tr = pose(affine(tr) @ (np.linalg.inv(self.last) @ back))
            self.last = back
        return tr


# ------------------------------------------------------------------------------- test scans
def first_kept(pts, H, W):
    kept, col, _ = proj_model.keep_mask(pts, H, W)
    i = int(np.flatnonzero(kept)[0])
    return i, int(col[i])


def skew_scan(pts, incre, period, W, direction=1, H=None, rounds=12):
    """The static scan `pts` (in the frame of the scan's start) as a sensor moving by `incre` during
    the scan records it: point i, fired at s_i in [0, 1), becomes q_i = T(s_i)^-1 p_i with T(s) =
    getTransformation(s * incre) and time_i = s_i * period.  s is made consistent with the column of
    the moved point, s = k(column(q)) / W with k counted from the first kept point in `direction`,
    by fixed-point iteration from the scan's own times (direction +1) or columns (-1).  The
    contraction factor is the parallax, so most points settle in three rounds; a point that sits on
    a column boundary (it flips between two columns for ever) or so near the sensor that its
    parallax factor approaches 1 has not settled after `rounds` and is left out of the scan (at most
    2 % of it; each point iterates on its own, so the rest are at their fixed points).  Both time
    sources then describe the same scan, and the deskew is its exact inverse up to float rounding.
    Returns (skewed scan, s, indices into `pts` of the points kept)."""
    H = int(pts["ring"].max()) + 1 if H is None else H
    incre = np.asarray(incre, np.float64)
    P = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)
    _, cf = first_kept(pts, H, W)  # fired at s = 0, so it does not move
    if direction == 1:
        s = pts["time"].astype(np.float64) / period
    else:
        s = column_k(direction, proj_model.column(pts["x"], pts["y"], W), cf, W) / W
    out = pts.copy()
    for _ in range(rounds):
        # T(s)^-1 p, vectorised: R(s)^T (p - t(s))
        ang, pos = s[:, None] * incre[None, :3], s[:, None] * incre[None, 3:]
        A, B, C, D, E, F = (np.cos(ang[:, 2]), np.sin(ang[:, 2]), np.cos(ang[:, 1]), np.sin(ang[:, 1]),
                            np.cos(ang[:, 0]), np.sin(ang[:, 0]))
        R = np.array([[A * C, A * D * F - B * E, B * F + A * D * E], [B * C, A * E + B * D * F, B * D * E - A * F],
                      [-D, C * F, C * E]]).transpose(2, 0, 1)
        Q = np.einsum("nji,nj->ni", R, P - pos)
        out["x"], out["y"], out["z"] = Q[:, 0], Q[:, 1], Q[:, 2]
        s_col = column_k(direction, proj_model.column(out["x"], out["y"], W), cf, W) / W
        settled = s_col == s  # `out` is the scan of s: these points' columns say the s they were moved by
        if settled.all():
            break
        s = np.where(settled, s, s_col)
    keep = np.flatnonzero(settled)
    assert len(keep) >= 0.98 * len(pts), len(keep) / len(pts)
    out["time"] = s * period
    out, s = out[keep].copy(), s[keep]
    assert first_kept(out, H, W)[1] == cf and s[first_kept(out, H, W)[0]] == 0
    return out, s, keep


def scan_direction(pts, W, period=0.1):
    """+1 or -1: the sense in which the scan's `time` sweeps its columns."""
    col = proj_model.column(pts["x"], pts["y"], W)
    t = pts["time"].astype(np.float64) / period
    err = {d: np.median(np.abs(column_k(d, col, col[0], W) / W - t)) for d in (1, -1)}
    return min(err, key=err.get), err
