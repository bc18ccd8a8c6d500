"""ctypes / numpy mirrors of the C-ABI types declared in include/fbr.h.

The layouts follow the reference's data model: ``POINT_XYZIRT`` is the PointXYZIRT payload of
/root/reference/src/imageProjection.cpp:8-21, ``POINT_XYZI`` is pcl::PointXYZI
(/root/reference/include/utility.h:55), ``FbrParams`` carries config/params.yaml plus the constants
mapOptmization.h hard-codes, ``FbrRegStats`` reports what registration() decided.
"""
import ctypes

import numpy as np

POINT_XYZIRT = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"),
     ("pad_", "<u2"), ("time", "<f4")], align=True)
assert POINT_XYZIRT.itemsize == 24

POINT_XYZI = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
assert POINT_XYZI.itemsize == 16

REG_STATS_FIELDS = ["status", "iterations", "converged", "degenerate", "n_sel", "n_corner_ds",
                    "n_surf_ds", "n_corner_map", "n_surf_map", "n_points", "n_corner", "n_surf"]
REG_STATS = np.dtype([(f, "<i4") for f in REG_STATS_FIELDS])

# IMU deskew (include/fbr.h "IMU deskew"): sensor_msgs/Imu fields, extrinsics, imuDeskewInfo table
IMU_QUEUE = 500  # queueLength, imageProjection.cpp:23
IMU_SAMPLE = np.dtype([("stamp", "<f8"), ("linear_acceleration", "<f8", 3), ("angular_velocity", "<f8", 3),
                       ("orientation", "<f8", 4)])
assert IMU_SAMPLE.itemsize == 88
IMU_EXTRINSICS = np.dtype([("ext_rot", "<f8", 9), ("ext_rpy", "<f8", 9)])
DESKEW_TABLE = np.dtype([("status", "<i4"), ("imu_available", "<i4"), ("imu_pointer_cur", "<i4"),
                         ("imu_roll_init", "<f4"), ("imu_pitch_init", "<f4"), ("imu_yaw_init", "<f4"),
                         ("time_scan_cur", "<f8"), ("imu_time", "<f8", IMU_QUEUE), ("imu_rot_x", "<f8", IMU_QUEUE),
                         ("imu_rot_y", "<f8", IMU_QUEUE), ("imu_rot_z", "<f8", IMU_QUEUE)], align=True)
assert DESKEW_TABLE.itemsize == 32 + 4 * 8 * IMU_QUEUE
FBR_DESKEW_READY, FBR_DESKEW_WAIT_IMU = 0, 1

# Motion deskew and the odometry guess (include/fbr.h "Motion deskew"): fbr_motion, fbr_odom_sample,
# fbr_odom_info, fbr_guess_state
FBR_MOTION_POSITION, FBR_MOTION_ROTATION = 1, 2
FBR_TIME_FIELD, FBR_TIME_COLUMN = 0, 1
MOTION = np.dtype([("flags", "<i4"), ("time_source", "<i4"), ("column_direction", "<i4"), ("reserved_", "<i4"),
                   ("incre", "<f4", 6), ("scan_period", "<f8")], align=True)
assert MOTION.itemsize == 48
ODOM_SAMPLE = np.dtype([("stamp", "<f8"), ("position", "<f8", 3), ("orientation", "<f8", 4), ("covariance0", "<f8")])
assert ODOM_SAMPLE.itemsize == 72
ODOM_INFO = np.dtype([("odom_available", "<i4"), ("odom_deskew_flag", "<i4"), ("initial_guess", "<f4", 6),
                      ("reset_id", "<i4"), ("reserved_", "<i4"), ("motion", MOTION)], align=True)
assert ODOM_INFO.itemsize == 88
GUESS_STATE = np.dtype([("reset_id", "<i4"), ("reserved_", "<i4"), ("last_imu", "<f4", 12)])
assert GUESS_STATE.itemsize == 56


def motion(incre, flags=FBR_MOTION_POSITION | FBR_MOTION_ROTATION, time_source=FBR_TIME_FIELD, scan_period=0.1,
           column_direction=1):
    """One MOTION record: incre = (rollIncre, pitchIncre, yawIncre, x, y, z) of the scan."""
    m = np.zeros(1, MOTION)
    m["flags"], m["time_source"], m["column_direction"] = flags, time_source, column_direction
    m["incre"], m["scan_period"] = np.asarray(incre, np.float32), scan_period
    return m[0]

# LIO-SAM keyframe store (include/fbr.h "LIO-SAM keyframe local map")
KEYPOSE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("roll", "<f4"),
                    ("pitch", "<f4"), ("yaw", "<f4"), ("pad_", "<f4"), ("time", "<f8")])
assert KEYPOSE.itemsize == 40


class FbrKeyframeParams(ctypes.Structure):
    _fields_ = [("search_radius", ctypes.c_float), ("pose_density", ctypes.c_float),
                ("loop_closure", ctypes.c_int32), ("submap_size", ctypes.c_int32),
                ("recent_window", ctypes.c_double)]


def keyframe_params(**kw):
    """fbr_keyframe_params_default (params.yaml:66-71, the 10 s window of mapOptmization.h:900)."""
    p = FbrKeyframeParams(50.0, 2.0, 0, 25, 10.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# loop closure (include/fbr.h "loop closure")
FBR_ICP_NOT_CONVERGED, FBR_ICP_ITERATIONS, FBR_ICP_TRANSFORM, FBR_ICP_ABS_MSE, FBR_ICP_REL_MSE, \
    FBR_ICP_NO_CORRESPONDENCES = range(6)
FBR_LOOP_CLOSED, FBR_LOOP_NO_CANDIDATE, FBR_LOOP_NOT_CONVERGED, FBR_LOOP_REJECTED_FITNESS = range(4)


class _Dictable(ctypes.Structure):
    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            if isinstance(v, ctypes.Array):
                v = np.array(v[:], np.float32)
            elif isinstance(v, _Dictable):
                v = v.as_dict()
            out[name] = v
        return out


class FbrIcpParams(_Dictable):
    _fields_ = [("max_correspondence_distance", ctypes.c_float), ("max_iterations", ctypes.c_int32),
                ("transformation_epsilon", ctypes.c_double), ("euclidean_fitness_epsilon", ctypes.c_double)]


class FbrLoopParams(_Dictable):
    _fields_ = [("search_radius", ctypes.c_float), ("search_time_diff", ctypes.c_float),
                ("search_num", ctypes.c_int32), ("fitness_score", ctypes.c_float),
                ("icp_leaf_size", ctypes.c_float), ("icp", FbrIcpParams)]


class FbrIcpResult(_Dictable):
    _fields_ = [("converged", ctypes.c_int32), ("convergence", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("n_correspondences", ctypes.c_int32), ("fitness", ctypes.c_double),
                ("transform", ctypes.c_float * 16)]


class FbrLoopResult(_Dictable):
    _fields_ = [("status", ctypes.c_int32), ("latest_id", ctypes.c_int32), ("closest_id", ctypes.c_int32),
                ("n_source", ctypes.c_int32), ("n_target", ctypes.c_int32), ("icp", FbrIcpResult),
                ("pose_corrected", ctypes.c_float * 6), ("pose_closest", ctypes.c_float * 6),
                ("between", ctypes.c_float * 16)]


class FbrLoopPair(_Dictable):
    """fbr_loop_pair: one entry of fbr_perform_loop_closures."""
    _fields_ = [("latest_id", ctypes.c_int32), ("closest_id", ctypes.c_int32), ("use_guess", ctypes.c_int32),
                ("pose_guess", ctypes.c_float * 6), ("reserved_", ctypes.c_int32)]


def icp_params(**kw):
    """performLoopClosure's "ICP Settings" (mapOptmization.h:689-694)."""
    p = FbrIcpParams(100.0, 100, 1e-6, 1e-6)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def loop_params(icp=None, **kw):
    """fbr_loop_params_default (params.yaml:72-75 and the ICP settings); `icp`: dict of
    fbr_icp_params overrides."""
    p = FbrLoopParams(15.0, 30.0, 25, 0.3, 0.0, icp_params(**(icp or {})))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# place recognition (include/fbr.h "place recognition")
FBR_SC_MAX_K = 16


class FbrScParams(_Dictable):
    _fields_ = [("n_ring", ctypes.c_int32), ("n_sector", ctypes.c_int32), ("max_radius", ctypes.c_float),
                ("lidar_height", ctypes.c_float), ("dist_threshold", ctypes.c_float), ("reserved_", ctypes.c_int32 * 3)]


class FbrScMatch(_Dictable):
    _fields_ = [("keyframe", ctypes.c_int32), ("shift", ctypes.c_int32), ("distance", ctypes.c_double),
                ("pose_guess", ctypes.c_float * 6), ("pad_", ctypes.c_float * 2)]


def sc_params(**kw):
    """fbr_sc_params_default: 20 rings x 60 sectors over 80 m, lidar height 2 m, dist_threshold 0.2."""
    p = FbrScParams(20, 60, 80.0, 2.0, 0.2)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# pose graph (include/fbr.h "pose graph")
FBR_PG_CONVERGED, FBR_PG_ITERATIONS, FBR_PG_STALLED, FBR_PG_NUMERICAL, FBR_PG_EMPTY = range(5)
FBR_PG_SOLVER_PCG, FBR_PG_SOLVER_DIRECT = range(2)
FBR_PG_ROBUST_NONE, FBR_PG_ROBUST_HUBER, FBR_PG_ROBUST_CAUCHY = range(3)
PG_SOLVERS = {"pcg": FBR_PG_SOLVER_PCG, "direct": FBR_PG_SOLVER_DIRECT}
PG_ROBUST = {"none": FBR_PG_ROBUST_NONE, "huber": FBR_PG_ROBUST_HUBER, "cauchy": FBR_PG_ROBUST_CAUCHY}


class FbrPgParams(_Dictable):
    _fields_ = [("max_iterations", ctypes.c_int32), ("max_pcg_iterations", ctypes.c_int32),
                ("rel_cost_tol", ctypes.c_double), ("abs_cost_tol", ctypes.c_double), ("pcg_rel_tol", ctypes.c_double),
                ("lambda_init", ctypes.c_double), ("lambda_factor", ctypes.c_double), ("lambda_max", ctypes.c_double),
                ("solver", ctypes.c_int32), ("robust", ctypes.c_int32), ("robust_scale", ctypes.c_float),
                ("max_work_mb", ctypes.c_int32)]


class FbrPgResult(_Dictable):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("trials", ctypes.c_int32),
                ("pcg_iterations", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("n_factors", ctypes.c_int32),
                ("n_loop_factors", ctypes.c_int32), ("pad_", ctypes.c_int32), ("cost_initial", ctypes.c_double),
                ("cost_final", ctypes.c_double), ("lambda", ctypes.c_double),
                ("max_translation_change", ctypes.c_double), ("max_rotation_change", ctypes.c_double)]


def pg_params(**kw):
    """fbr_pg_params_default: 30 LM steps, 200 PCG iterations, GTSAM's 1e-5 error tolerances, PCG 1e-8,
    lambda 1e-5 x 10 up to 1e10; the conjugate-gradient solver and no robust option.  solver and
    robust also take their names ("direct"; "huber", "cauchy")."""
    p = FbrPgParams(30, 200, 1e-5, 1e-5, 1e-8, 1e-5, 10.0, 1e10)
    for k, v in kw.items():
        if k == "solver" and isinstance(v, str):
            v = PG_SOLVERS[v]
        if k == "robust" and isinstance(v, str):
            v = PG_ROBUST[v]
        setattr(p, k, v)
    return p


class FbrPgMarginalParams(_Dictable):
    _fields_ = [("rhs_chunk", ctypes.c_int32), ("reserved_", ctypes.c_int32 * 3), ("max_work_bytes", ctypes.c_int64)]


class FbrPgMarginalResult(_Dictable):
    _fields_ = [("status", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("n_loop_factors", ctypes.c_int32),
                ("n_out", ctypes.c_int32), ("work_bytes", ctypes.c_int64)]


def pg_marginal_params(**kw):
    """fbr_pg_marginal_params_default: rhs_chunk 0 (48 columns per pass), max_work_bytes 0 (2 GiB)."""
    p = FbrPgMarginalParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# global map (include/fbr.h "global map")
FBR_GMAP_SAVE_GLOBAL = 1


class FbrGmapParams(_Dictable):
    _fields_ = [("corner_leaf", ctypes.c_float), ("surf_leaf", ctypes.c_float), ("wide", ctypes.c_int32),
                ("keep_raw", ctypes.c_int32), ("reserved_", ctypes.c_int32 * 4)]


class FbrGmapResult(_Dictable):
    _fields_ = [("n_keyframes", ctypes.c_int64), ("n_corner_raw", ctypes.c_int64), ("n_surf_raw", ctypes.c_int64),
                ("n_corner", ctypes.c_int64), ("n_surf", ctypes.c_int64), ("n_dropped", ctypes.c_int64),
                ("corner_overflow", ctypes.c_int32), ("surf_overflow", ctypes.c_int32),
                ("corner_wide", ctypes.c_int32), ("surf_wide", ctypes.c_int32)]


def gmap_params(**kw):
    """fbr_gmap_params_default: the context's mapping leaves (0), PCL semantics (wide = 0), no raw clouds."""
    p = FbrGmapParams(0.0, 0.0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# pose scoring (include/fbr.h "pose scoring")
FBR_POSE_SEARCH_MAX = 1 << 20


class FbrScoreParams(_Dictable):
    _fields_ = [("gate", ctypes.c_float), ("use_crop", ctypes.c_int32), ("pose_chunk", ctypes.c_int32),
                ("reserved_", ctypes.c_int32 * 5)]


class FbrPoseLattice(_Dictable):
    _fields_ = [("half", ctypes.c_float * 4), ("step", ctypes.c_float * 4)]


# fbr_pose_score as a record array: one per pose
POSE_SCORE = np.dtype([("n", np.int32, 2), ("n_in", np.int32, 2), ("sum_d2", np.float64, 2), ("fitness", np.float64)])
assert POSE_SCORE.itemsize == 40


def score_params(**kw):
    """fbr_score_params_default: gate 1 m, registration's crop box, pose_chunk 0 (1024 poses per launch)."""
    p = FbrScoreParams(1.0, 1, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pose_lattice(half=(0.0, 0.0, 0.0, 0.0), step=(0.0, 0.0, 0.0, 0.0)):
    """fbr_pose_lattice over x, y, z (m) and yaw (rad): offsets i * step for |i| <= floor(half / step)."""
    return FbrPoseLattice((ctypes.c_float * 4)(*half), (ctypes.c_float * 4)(*step))


# registration information (include/fbr.h "registration information")
FBR_INFO_NO_ROWS = 1
FBR_INFO_FEW_ROWS = 2
FBR_INFO_BAD_POSE = 4
FBR_INFO_NOT_REGISTERED = 8


class FbrInfoParams(_Dictable):
    _fields_ = [("eig_floor", ctypes.c_double), ("unobserved_variance", ctypes.c_double), ("sigma2", ctypes.c_double),
                ("pose_chunk", ctypes.c_int32), ("reserved_", ctypes.c_int32 * 5)]


# fbr_reg_info as a record array: one per pose or batch job
REG_INFO = np.dtype([("H", np.float64, (6, 6)), ("g", np.float64, 6), ("rss", np.float64), ("sigma2", np.float64),
                     ("eig", np.float64, 6), ("evec", np.float64, (6, 6)), ("cov", np.float64, (6, 6)),
                     ("cov_tangent", np.float64, (6, 6)), ("var_tangent", np.float64, 6), ("n_rows", np.int32, 2),
                     ("n_query", np.int32, 2), ("rank", np.int32), ("flags", np.int32)])
assert REG_INFO.itemsize == 1336


def info_params(**kw):
    """fbr_info_params_default: eigenvalue floor 100, unobserved variance 1e4 ("unknown"), sigma2 from the
    residuals (0), pose_chunk 0 (1024 poses or jobs per launch)."""
    p = FbrInfoParams(100.0, 1e4, 0.0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


FBR_OK = 0
FBR_REG_OK = 0
FBR_REG_NOT_ENOUGH_FEATURES = 1
FBR_REG_SKIPPED_INTERVAL = 2
FBR_REG_FEATURE_CAPACITY = 3  # batch job over the device feature capacity: pose = guess


class FbrParams(ctypes.Structure):
    _fields_ = [
        ("n_scan", ctypes.c_int32),
        ("horizon_scan", ctypes.c_int32),
        ("edge_threshold", ctypes.c_float),
        ("surf_threshold", ctypes.c_float),
        ("edge_feature_min_valid_num", ctypes.c_int32),
        ("surf_feature_min_valid_num", ctypes.c_int32),
        ("odometry_surf_leaf_size", ctypes.c_float),
        ("mapping_corner_leaf_size", ctypes.c_float),
        ("mapping_surf_leaf_size", ctypes.c_float),
        ("z_tollerance", ctypes.c_float),
        ("rotation_tollerance", ctypes.c_float),
        ("number_of_cores", ctypes.c_int32),
        ("mapping_process_interval", ctypes.c_double),
        ("crop_half", ctypes.c_float * 3),
        ("max_iterations", ctypes.c_int32),
        ("max_points_per_scan", ctypes.c_int32),
        ("max_batch", ctypes.c_int32),
        ("exact_voxel_order", ctypes.c_int32),
        ("pipeline_depth", ctypes.c_int32),
        ("reserved_", ctypes.c_int32 * 2),
    ]


class FbrRegStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int32) for f in REG_STATS_FIELDS]

    def as_dict(self):
        return {f: getattr(self, f) for f in REG_STATS_FIELDS}


def default_params(n_scan=16, horizon_scan=1800, **overrides):
    """fbr_params_default(): params.yaml values + the reference's hard-coded constants."""
    p = FbrParams()
    p.n_scan = n_scan
    p.horizon_scan = horizon_scan
    p.edge_threshold = 1.0
    p.surf_threshold = 0.1
    p.edge_feature_min_valid_num = 10
    p.surf_feature_min_valid_num = 100
    p.odometry_surf_leaf_size = 0.4
    p.mapping_corner_leaf_size = 0.2
    p.mapping_surf_leaf_size = 0.4
    p.z_tollerance = 1000.0
    p.rotation_tollerance = 1000.0
    p.number_of_cores = 4
    p.mapping_process_interval = 0.15
    p.crop_half[0], p.crop_half[1], p.crop_half[2] = 30.0, 30.0, 10.0
    p.max_iterations = 30
    p.max_points_per_scan = n_scan * horizon_scan
    p.max_batch = 1
    for k, v in overrides.items():
        if k == "crop_half":
            for i in range(3):
                p.crop_half[i] = v[i]
        else:
            setattr(p, k, v)
    return p


def ptr(a, ctype=ctypes.c_void_p):
    """Raw pointer of a contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return ctypes.cast(a.ctypes.data, ctype)


# ---- sensor_msgs/PointCloud2 (include/fbr.h "PointCloud2 wire format") ----
PF_INT8, PF_UINT8, PF_INT16, PF_UINT16, PF_INT32, PF_UINT32, PF_FLOAT32, PF_FLOAT64 = range(1, 9)
FBR_ERR_MSG = -8
FBR_MSG_NO_TIME, FBR_MSG_RING_UNMAPPED, FBR_MSG_XYZI_UNMAPPED = 1, 2, 4
_PF_OF_NUMPY = {"i1": PF_INT8, "u1": PF_UINT8, "i2": PF_INT16, "u2": PF_UINT16, "i4": PF_INT32,
                "u4": PF_UINT32, "f4": PF_FLOAT32, "f8": PF_FLOAT64}


class FbrPointField(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("offset", ctypes.c_uint32), ("datatype", ctypes.c_uint8),
                ("count", ctypes.c_uint32)]


class FbrPointCloud2(ctypes.Structure):
    _fields_ = [("height", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("fields", ctypes.POINTER(FbrPointField)), ("n_fields", ctypes.c_int32),
                ("is_bigendian", ctypes.c_uint8), ("point_step", ctypes.c_uint32),
                ("row_step", ctypes.c_uint32), ("data", ctypes.c_void_p), ("data_size", ctypes.c_uint64),
                ("is_dense", ctypes.c_uint8)]


class PointCloud2:
    """A sensor_msgs/PointCloud2 view for the C-ABI: keeps the byte buffer and field names alive.

    fields: list of (name, offset, datatype, count).  `data` is bytes-like of at least
    (height-1)*row_step + width*point_step bytes."""

    def __init__(self, data, fields, width, height=1, point_step=None, row_step=None, is_dense=True):
        self.buf = np.frombuffer(bytes(data), np.uint8)
        self.fields = [(str(n), int(o), int(t), int(c)) for n, o, t, c in fields]
        self._names = [n.encode() for n, _, _, _ in self.fields]
        self._fa = (FbrPointField * max(len(self.fields), 1))()
        for k, ((_, o, t, c), nm) in enumerate(zip(self.fields, self._names)):
            self._fa[k] = FbrPointField(nm, o, t, c)
        ps = point_step if point_step is not None else (len(self.buf) // max(width * height, 1))
        m = FbrPointCloud2()
        m.height, m.width = height, width
        m.fields = ctypes.cast(self._fa, ctypes.POINTER(FbrPointField))
        m.n_fields = len(self.fields)
        m.is_bigendian = 0
        m.point_step = ps
        m.row_step = row_step if row_step is not None else ps * width
        m.data = self.buf.ctypes.data if len(self.buf) else None
        m.data_size = len(self.buf)
        m.is_dense = 1 if is_dense else 0
        self.c = m

    @classmethod
    def from_array(cls, arr, height=1, is_dense=True):
        """Message whose points are the records of a numpy structured array (fields by dtype)."""
        arr = np.ascontiguousarray(arr)
        fields = []
        for name in arr.dtype.names:
            dt, off = arr.dtype.fields[name][:2]
            base, shape = (dt.subdtype if dt.subdtype else (dt, ()))
            count = int(np.prod(shape)) if shape else 1
            fields.append((name, off, _PF_OF_NUMPY[base.str[1:]], count))
        return cls(arr.tobytes(), fields, width=len(arr) // height, height=height,
                   point_step=arr.dtype.itemsize, is_dense=is_dense)
