/* fbr.h — C-ABI of the MI355X-native feature-based scan-to-map registration path.
 *
 * Drop-in boundary for the per-scan hot loop of qpc001/Feature_Base_Pointcloud_Registration
 * (a LIO-SAM-derived localiser).  The reference's "operator API" for this path is in-process C++:
 *
 *   ImageProjection::cloudHandler()            src/imageProjection.cpp:182-226
 *     projectPointCloud() / cloudExtraction()  src/imageProjection.cpp:583-670
 *   FeatureExtraction::featureExtra()          src/featureExtraction.h:79-103
 *   mapOptimization::registration()            src/mapOptmization.h:263-343
 *   mapOptimization::allocateMemory() (map)    src/mapOptmization.h:245-260
 *
 * Each entry point below names the reference function it replaces.  Conventions:
 *   - plain C types only; host buffers are caller-owned; device memory is owned by the ctx;
 *   - every function returns an int status: 0 = FBR_OK, < 0 = error (fbr_strerror());
 *   - a ctx is bound to one HIP device and one HIP stream and is not thread-safe
 *     (one ctx per host thread and device, as the reference runs one scan at a time);
 *   - poses are the reference's transformTobeMapped layout [roll, pitch, yaw, x, y, z]
 *     (mapOptmization.h:131); fbr_affine_from_pose / fbr_pose_from_affine convert to and from the
 *     Eigen::Affine3f the reference's registration() takes, with PCL's exact formulas.
 */
#ifndef FBR_H_
#define FBR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBR_ABI_VERSION 4  /* 4: fbr_batch_allgather takes wait_stream (the caller's reader of recv);
                              3: fbr_params.exact_voxel_order / pipeline_depth (were reserved_[0..1]);
                              2: fbr_selftest_math writes 6 floats per element (was 4) */

/* ---- status codes ------------------------------------------------------------------------- */
#define FBR_OK 0
#define FBR_ERR_INVALID_ARG (-1)  /* null pointer, negative size, bad parameter            */
#define FBR_ERR_HIP (-2)          /* a HIP runtime call failed                              */
#define FBR_ERR_NO_MAP (-3)       /* registration requested before fbr_set_map()           */
#define FBR_ERR_CAPACITY (-4)     /* input larger than the ctx was created for              */
#define FBR_ERR_UNSUPPORTED (-5)  /* configuration outside what the kernels handle          */
#define FBR_ERR_NO_DEVICE (-6)    /* no HIP device / extension not usable                   */
#define FBR_ERR_STATE (-7)        /* call order violated (e.g. features before projection)  */
#define FBR_ERR_MSG (-8)          /* PointCloud2 rejected by cachePointCloud's checks: not
                                     is_dense, or no "ring" field (imageProjection.cpp:256-281,
                                     where the reference calls ros::shutdown())               */

/* ---- registration outcome (fbr_reg_stats.status) -------------------------------------------- */
#define FBR_REG_OK 0                    /* scan2MapOptimization ran                           */
#define FBR_REG_NOT_ENOUGH_FEATURES 1   /* mapOptmization.h:1410/1440 gate: pose left at guess */
#define FBR_REG_SKIPPED_INTERVAL 2      /* mapOptmization.h:279 mappingProcessInterval gate    */
#define FBR_REG_FEATURE_CAPACITY 3      /* batch job: features exceeded the device capacity;   */
                                        /* its pose is left at the guess (single-scan calls    */
                                        /* return FBR_ERR_UNSUPPORTED instead)                 */

/* Raw lidar point: the PointXYZIRT payload of imageProjection.cpp:8-21 (x,y,z,intensity f32,
 * ring u16, time f32), laid out with natural alignment (24 bytes). */
typedef struct fbr_point_xyzirt {
  float x, y, z, intensity;
  uint16_t ring;
  uint16_t pad_;
  float time;
} fbr_point_xyzirt;

/* Work point: pcl::PointXYZI payload (include/utility.h:55). */
typedef struct fbr_point_xyzi {
  float x, y, z, intensity;
} fbr_point_xyzi;

/* Tunables.  Defaults (fbr_params_default) are config/params.yaml plus the constants the
 * reference hard-codes (SURVEY §5 "Config / flags"). */
typedef struct fbr_params {
  int32_t n_scan;                    /* N_SCAN                       params.yaml:19        */
  int32_t horizon_scan;              /* Horizon_SCAN                 params.yaml:20        */
  float edge_threshold;              /* edgeThreshold 1.0            params.yaml:45        */
  float surf_threshold;              /* surfThreshold 0.1            params.yaml:46        */
  int32_t edge_feature_min_valid_num;/* 10                           params.yaml:47        */
  int32_t surf_feature_min_valid_num;/* 100                          params.yaml:48        */
  float odometry_surf_leaf_size;     /* 0.4 per-ring surf VoxelGrid  params.yaml:51        */
  float mapping_corner_leaf_size;    /* 0.2                          params.yaml:52        */
  float mapping_surf_leaf_size;      /* 0.4                          params.yaml:53        */
  float z_tollerance;                /* 1000                         params.yaml:56        */
  float rotation_tollerance;         /* 1000                         params.yaml:57        */
  int32_t number_of_cores;           /* 4 (CPU paths only)           params.yaml:60        */
  double mapping_process_interval;   /* 0.15 s                       params.yaml:61        */
  float crop_half[3];                /* 30, 30, 10 m local-map box   mapOptmization.h:286  */
  int32_t max_iterations;            /* 30 Gauss-Newton iterations   mapOptmization.h:1417 */
  int32_t max_points_per_scan;       /* device capacity: raw points per scan               */
  int32_t max_batch;                 /* device capacity: scans per device batch            */
  int32_t exact_voxel_order;         /* 0: every VoxelGrid sums a voxel's points in index order
                                        (centroids to float rounding, the fast default); 1: in
                                        std::sort's order, as PCL does (bit-identical centroids and
                                        poses vs the oracle, ~0.45x the batch throughput)        */
  int32_t pipeline_depth;            /* batch launch slots 1..3 (0 = default 3; forced to 1 when
                                        max_batch = 1): launch n's front end overlaps the
                                        Gauss-Newton tails of up to depth-1 launches before it    */
  int32_t reserved_[2];
} fbr_params;

/* Per-scan registration statistics. */
typedef struct fbr_reg_stats {
  int32_t status;       /* FBR_REG_*                                                       */
  int32_t iterations;   /* LMOptimization calls made (<= max_iterations)                   */
  int32_t converged;    /* 1 if the loop ended on the 0.05 deg / 0.05 cm test               */
  int32_t degenerate;   /* isDegenerate after the last LMOptimization call                  */
  int32_t n_sel;        /* correspondences in the last LMOptimization call                  */
  int32_t n_corner_ds;  /* laserCloudCornerLastDSNum                                        */
  int32_t n_surf_ds;    /* laserCloudSurfLastDSNum                                          */
  int32_t n_corner_map; /* laserCloudCornerFromMapDSNum (cropped local map)                 */
  int32_t n_surf_map;   /* laserCloudSurfFromMapDSNum                                       */
  int32_t n_points;     /* valid projected points (cloud_deskewed size)                     */
  int32_t n_corner;     /* corner features before DS                                        */
  int32_t n_surf;       /* surface features before DS                                       */
} fbr_reg_stats;

typedef struct fbr_ctx fbr_ctx;

/* ---- sensor_msgs/PointCloud2 wire format ------------------------------ */
/* sensor_msgs/PointField datatypes */
#define FBR_PF_INT8 1
#define FBR_PF_UINT8 2
#define FBR_PF_INT16 3
#define FBR_PF_UINT16 4
#define FBR_PF_INT32 5
#define FBR_PF_UINT32 6
#define FBR_PF_FLOAT32 7
#define FBR_PF_FLOAT64 8

typedef struct fbr_point_field { /* sensor_msgs/PointField */
  const char* name;
  uint32_t offset;
  uint8_t datatype;              /* FBR_PF_* */
  uint32_t count;
} fbr_point_field;

typedef struct fbr_pointcloud2 { /* sensor_msgs/PointCloud2 without the header */
  uint32_t height, width;
  const fbr_point_field* fields;
  int32_t n_fields;
  uint8_t is_bigendian;          /* ignored, as pcl::fromROSMsg does (host byte order assumed) */
  uint32_t point_step, row_step;
  const uint8_t* data;
  uint64_t data_size;            /* bytes at data (>= (height-1)*row_step + width*point_step) */
  uint8_t is_dense;
} fbr_pointcloud2;

/* msg_flags bits reported by the *_msg entry points (warnings, the call still succeeds) */
#define FBR_MSG_NO_TIME 1        /* no "time" field: deskewFlag = -1, ROS_WARN (:285-298); time = 0 */
#define FBR_MSG_RING_UNMAPPED 2  /* "ring" exists but is not UINT16 x1: fromROSMsg leaves ring = 0 */
#define FBR_MSG_XYZI_UNMAPPED 4  /* x, y, z or intensity missing / not FLOAT32 x1: left 0          */

void fbr_params_default(fbr_params* p);
const char* fbr_strerror(int status);
int fbr_abi_version(void);
int fbr_device_count(int* count);

/* Create / destroy a context on HIP device `hip_device` (ParamServer + member construction,
 * utility.h:146-212, featureExtraction.h:48-77, mapOptmization.h:153-196). */
int fbr_create(fbr_ctx** out, const fbr_params* p, int hip_device);
int fbr_destroy(fbr_ctx* ctx);

/* Load the prior global feature map (already read from cloudCorner.pcd / cloudSurf.pcd) and
 * apply the start-up VoxelGrid (corner leaf mapping_corner_leaf_size, surf leaf
 * mapping_surf_leaf_size), replacing mapOptmization.h:245-260.  Builds the device search grid. */
int fbr_set_map(fbr_ctx* ctx, const fbr_point_xyzi* corner, int64_t n_corner,
                const fbr_point_xyzi* surf, int64_t n_surf);
/* pcl::io::loadPCDFile(HOME + savePCDDirectory + "cloudCorner.pcd" / "cloudSurf.pcd") followed by
 * fbr_set_map — the whole start-up block mapOptmization.h:245-260 (host-side PCD parsing). */
int fbr_load_map(fbr_ctx* ctx, const char* corner_pcd, const char* surf_pcd);

/* PCD v0.7 I/O for PointXYZI clouds (host only, no device needed).
 * fbr_pcd_read replaces pcl::io::loadPCDFile<PointXYZI> (mapOptmization.h:247-248): DATA ascii,
 * binary and binary_compressed (LZF); x, y, z and intensity are taken by name from any field
 * layout (F/U/I types, other fields skipped, missing intensity = 0).  Call with out == NULL to get
 * the point count in *n, then with a buffer of cap >= *n points (FBR_ERR_CAPACITY otherwise).
 * fbr_pcd_write_ascii replaces pcl::io::savePCDFileASCII (mapOptmization.h:511-515): PCL's header
 * and 8 significant digits per value.  fbr_pcd_write_binary writes DATA binary (exact floats). */
int fbr_pcd_read(const char* path, fbr_point_xyzi* out, int64_t cap, int64_t* n);
int fbr_pcd_write_ascii(const char* path, const fbr_point_xyzi* points, int64_t n);
int fbr_pcd_write_binary(const char* path, const fbr_point_xyzi* points, int64_t n);

/* cachePointCloud's conversion and checks (imageProjection.cpp:255-298) on the host:
 * pcl::fromROSMsg<PointXYZIRT> (fields mapped by name with matching datatype and count, points in
 * row-major order, unmapped fields 0), then the is_dense and "ring" checks (FBR_ERR_MSG) and the
 * "time" check (FBR_MSG_NO_TIME).  out == NULL queries *n.  The reference runs the ring/time
 * checks on the first message only (static flags); these entry points check every message. */
int fbr_msg_to_points(const fbr_pointcloud2* msg, fbr_point_xyzirt* out, int64_t cap, int64_t* n,
                      int32_t* msg_flags);
/* pcl::toROSMsg of a PointXYZI cloud (publishCloud, utility.h:255-264): height 1, width n,
 * fields x@0 y@4 z@8 intensity@16 (FLOAT32 x1), point_step 32, row_step 32n, with PCL's padding
 * (1.0f at offset 12, zeros after intensity).  data_out holds 32*n bytes. */
int fbr_points_to_msg_data(const fbr_point_xyzi* points, int64_t n, uint8_t* data_out);

/* Device variants of fbr_project / fbr_process_scan that take the raw PointCloud2: the message
 * bytes are copied to HBM as they are and unpacked by a kernel (field mapping as
 * fbr_msg_to_points), so the host does no per-point work (cachePointCloud + cloudHandler,
 * imageProjection.cpp:182-226). */
int fbr_project_msg(fbr_ctx* ctx, const fbr_pointcloud2* msg, int32_t* start_ring, int32_t* end_ring,
                    int32_t* col_ind, float* range, fbr_point_xyzi* cloud, int64_t* n_out,
                    int32_t* msg_flags);
int fbr_process_msg(fbr_ctx* ctx, const fbr_pointcloud2* msg, double stamp, float pose_inout[6],
                    fbr_reg_stats* stats, int32_t* msg_flags);

/* ---- IMU deskew --------------------------------------------------------
 * The reference carries LIO-SAM's IMU deskew but calls it nowhere: deskewInfo() is commented out
 * in cloudHandler (imageProjection.cpp:189-191), so imuAvailable stays 0 and deskewPoint() is the
 * identity (:548-549).  These entry points restore the path as it runs with that call enabled:
 *   fbr_imu_convert      imuConverter (utility.h:219-253), applied by imuHandler to each sample
 *   fbr_imu_deskew_info  deskewInfo + imuDeskewInfo (imageProjection.cpp:303-393) on the host:
 *                        a serial pass over the ~20 queued samples that builds the scan's table
 *   fbr_set_deskew       hands tables to the device: the compaction kernel then applies
 *                        deskewPoint / findRotation (:494-580) to every kept point, and
 *                        transformUpdate (mapOptmization.h:1444-1474) slerps roll and pitch towards
 *                        imuRollInit / imuPitchInit.
 * findPosition is all-zero in the reference (:528-542, positional deskew commented out), and the
 * odometry half of deskewInfo only fills initial-guess fields read by the disabled
 * updateInitialGuess; neither has an observable effect on this path while it stays off.  The
 * motion entry points below (fbr_set_motion and its companions) switch both on. */
#define FBR_IMU_QUEUE 500 /* queueLength, imageProjection.cpp:23 */

typedef struct fbr_imu_sample { /* the sensor_msgs/Imu fields the path reads */
  double stamp;                 /* header.stamp.toSec()                                  */
  double linear_acceleration[3];
  double angular_velocity[3];
  double orientation[4];        /* x, y, z, w                                             */
} fbr_imu_sample;

typedef struct fbr_imu_extrinsics { /* ParamServer extrinsics (utility.h:172-178), row-major */
  double ext_rot[9];                /* extrinsicRot                                          */
  double ext_rpy[9];                /* extrinsicRPY (-> extQRPY)                             */
} fbr_imu_extrinsics;

/* fbr_deskew_table.status */
#define FBR_DESKEW_READY 0    /* deskewInfo() returned true: the scan is processed                */
#define FBR_DESKEW_WAIT_IMU 1 /* deskewInfo() returned false (the IMU queue does not cover the
                                 scan, :310-314): the reference's cloudHandler drops the scan     */

typedef struct fbr_deskew_table { /* imuDeskewInfo() state of one scan (imageProjection.cpp:52-57) */
  int32_t status;                 /* FBR_DESKEW_*                                                   */
  int32_t imu_available;          /* cloudInfo.imuAvailable                                         */
  int32_t imu_pointer_cur;        /* imuPointerCur                                                  */
  float imu_roll_init, imu_pitch_init, imu_yaw_init; /* cloudInfo.imu{Roll,Pitch,Yaw}Init          */
  double time_scan_cur;           /* timeScanCur                                                    */
  double imu_time[FBR_IMU_QUEUE]; /* imuTime                                                        */
  double imu_rot_x[FBR_IMU_QUEUE], imu_rot_y[FBR_IMU_QUEUE], imu_rot_z[FBR_IMU_QUEUE];
} fbr_deskew_table;

/* imuConverter: acceleration and angular velocity rotated by extrinsicRot, orientation =
 * extQRPY * q (Eigen, double).  FBR_ERR_INVALID_ARG for the |q| < 0.1 "please use a 9-axis IMU"
 * case, where the reference shuts the node down (:246-250). */
int fbr_imu_convert(const fbr_imu_extrinsics* ext, const fbr_imu_sample* in, fbr_imu_sample* out);
/* deskewInfo()'s IMU half on a queue of converted samples in arrival order.  *n_pop receives the
 * number of leading samples imuDeskewInfo pops (stamp < time_scan_cur - 0.01, :328-335), which the
 * caller removes from its queue (0 when the scan is dropped: deskewInfo returns before popping).
 * The table's imu_*_init fields are only overwritten when a sample at or before time_scan_cur
 * remains (:354-355): pass the previous scan's table to keep the reference's carry-over.
 * FBR_ERR_CAPACITY if the scan needs more than FBR_IMU_QUEUE samples (the reference overruns its
 * arrays there). */
int fbr_imu_deskew_info(const fbr_imu_sample* imu_queue, int64_t n_imu, double time_scan_cur,
                        double time_scan_next, fbr_deskew_table* out, int64_t* n_pop);
/* Deskew tables for the following calls: job j of a staged batch uses tables[j] (j < n_tables),
 * the single-scan calls use tables[0].  tables == NULL or n_tables == 0 restores the reference's
 * runtime behaviour (no deskew, imuAvailable = 0).  A PointCloud2 without a "time" field disables
 * the point deskew for that call (deskewFlag = -1, :296-297, :548) but not the IMU update. */
int fbr_set_deskew(fbr_ctx* ctx, const fbr_deskew_table* tables, int n_tables);

/* ---- Motion deskew from odometry or the pose chain, and the odometry guess -------------------
 * The rest of LIO-SAM's motion path, which the reference carries switched off:
 *   fbr_odom_deskew_info     odomDeskewInfo (imageProjection.cpp:395-491): the initial-guess fields,
 *                            odomAvailable, and the scan's begin-to-end increment of
 *                            transBegin^-1 * transEnd as a fbr_motion
 *   fbr_motion_from_poses    the same record from the last two registration results (constant
 *                            velocity), for hosts without odometry, with the predicted next guess
 *   fbr_update_initial_guess updateInitialGuess (mapOptmization.h:799-855) on a caller-owned state
 *   fbr_set_motion           hands fbr_motion records to the device: deskewPoint (:545-580) then runs
 *                            with findPosition's commented body live (:528-542)
 * The arithmetic of one point (csrc/fbr_motion.h, the same code on the host and in the kernels):
 *   ratio   FBR_TIME_FIELD:  (float)((double)point.time / scan_period)
 *           FBR_TIME_COLUMN: (float)k / (float)W, k = (column_direction * (col - col_first)) mod W
 *                            in [0, W), col the kept cell's column, col_first the column of the
 *                            scan's first kept point in input order (a spinning sensor sweeps its
 *                            columns at a constant rate, as LOAM / LeGO-LOAM take it)
 *   pos     ratio * incre[3..5] with FBR_MOTION_POSITION, else 0
 *   rot     findRotation's when the job has an IMU table with imu_available (fbr_set_deskew; it
 *           reads the point's time whatever time_source says); else ratio * incre[0..2] with
 *           FBR_MOTION_ROTATION; else 0
 *   transFinal = getTransformation(pos, rot); transStartInverse = transFinal(first point).inverse()
 *   (Eigen: t' = (-L^-1) * t); transBt = transStartInverse * transFinal (t = L1 * t2 + t1); float,
 *   3-term sums as x0 + (x1 + x2), no FMA.
 * Only the cloud changes (and the feature clouds taken from it): range, col_ind and start/end_ring
 * stay the raw point's (rangeMat is written before deskewPoint, :633-635).  With FBR_TIME_COLUMN the
 * transform depends on the column alone, so it needs neither the `time` field nor the 24-B scans: it
 * runs on a batch's 16-B device records and on a PointCloud2 without "time", where the IMU deskew
 * and FBR_TIME_FIELD are disabled (FBR_MSG_NO_TIME). */
#define FBR_MOTION_POSITION 1 /* findPosition live                                               */
#define FBR_MOTION_ROTATION 2 /* rotation from the increment when the job has no IMU table       */
#define FBR_TIME_FIELD 0
#define FBR_TIME_COLUMN 1
typedef struct fbr_motion {
  int32_t flags, time_source, column_direction /* +1 | -1, COLUMN only */, reserved_;
  float incre[6];     /* rollIncre, pitchIncre, yawIncre, odomIncreX, Y, Z of transBegin^-1 * transEnd */
  double scan_period; /* FIELD only; > 0 */
} fbr_motion;         /* 48 bytes */

typedef struct fbr_odom_sample { /* the nav_msgs/Odometry fields the path reads */
  double stamp;                  /* header.stamp.toSec()      */
  double position[3];            /* pose.pose.position        */
  double orientation[4];         /* x, y, z, w                */
  double covariance0;            /* pose.covariance[0]: the IMU pre-integration reset id */
} fbr_odom_sample;               /* 72 bytes */

typedef struct fbr_odom_info {
  int32_t odom_available;   /* cloudInfo.odomAvailable                                       */
  int32_t odom_deskew_flag; /* odomDeskewFlag                                                */
  float initial_guess[6];   /* initialGuess{Roll, Pitch, Yaw, X, Y, Z}                       */
  int32_t reset_id;         /* cloudInfo.imuPreintegrationResetId                            */
  int32_t reserved_;
  fbr_motion motion;        /* flags 0 unless odom_deskew_flag: the caller ORs in FBR_MOTION_* */
} fbr_odom_info;            /* 88 bytes */

typedef struct fbr_guess_state { /* what updateInitialGuess keeps between scans */
  int32_t reset_id;              /* the mapping side's imuPreintegrationResetId (caller-owned) */
  int32_t reserved_;
  float last_imu[12];            /* lastImuTransformation, row-major 3x4 */
} fbr_guess_state;               /* 56 bytes */

/* odomDeskewInfo on a queue of samples in arrival order.  *n_pop receives the number of leading
 * samples it pops (stamp < time_scan_cur - 0.01).  out->motion has time_source FBR_TIME_FIELD,
 * column_direction +1, scan_period = time_scan_next - time_scan_cur and, when odom_deskew_flag is
 * set, the increment; its flags are 0 (the reference runs with the path off): set
 * FBR_MOTION_POSITION (| FBR_MOTION_ROTATION) and the time source before fbr_set_motion. */
int fbr_odom_deskew_info(const fbr_odom_sample* odom_queue, int64_t n_odom, double time_scan_cur,
                         double time_scan_next, fbr_odom_info* out, int64_t* n_pop);
/* Constant velocity from two registered poses {roll, pitch, yaw, x, y, z} taken dt apart: the six
 * components of prev^-1 * cur scaled by scan_period / dt are the increment (flags POSITION |
 * ROTATION, FIELD time, direction +1), and scaled by dt_next / dt they predict the next scan's
 * guess, guess_out = cur * getTransformation(...).  out or guess_out may be NULL.
 * FBR_ERR_INVALID_ARG for dt <= 0 or a non-finite input. */
int fbr_motion_from_poses(const float prev[6], const float cur[6], double dt, double scan_period,
                          double dt_next, fbr_motion* out, float guess_out[6]);
/* updateInitialGuess on pose_inout (transformTobeMapped): the first frame (have_keyframes == 0)
 * from the IMU attitude of `table`; the odometry guess while odom->odom_available and
 * odom->reset_id == state->reset_id; else, with table->imu_available, the IMU rotation increment
 * since the last call applied to the previous pose.  odom or table may be NULL (not available);
 * with neither branch taken the pose is left as it is.  Touches no context. */
int fbr_update_initial_guess(fbr_guess_state* state, const fbr_odom_info* odom, const fbr_deskew_table* table,
                             int have_keyframes, int use_imu_heading, float pose_inout[6]);
/* Motion records for the following calls, addressed as fbr_set_deskew's tables: job j of a staged
 * batch uses motions[j] (j < n), the single-scan calls use motions[0]; NULL or n == 0 turns the
 * path off.  A job with flags == 0 is untouched.  FBR_ERR_INVALID_ARG for unknown flags or
 * time_source, a column_direction other than +1 / -1, scan_period <= 0 with FBR_TIME_FIELD, or a
 * non-finite increment.  With FBR_TIME_FIELD a PointCloud2 without "time" disables the job's motion
 * deskew for that call, and a batch staged as 16-B records answers FBR_ERR_STATE at launch (stage
 * it again); with FBR_TIME_COLUMN neither applies.  fbr_reset_stream keeps the records. */
int fbr_set_motion(fbr_ctx* ctx, const fbr_motion* motions, int n);

/* ---- LIO-SAM keyframe local map ------------------------------------
 * The reference's mapping back-end (laserCloudInfoHandler, mapOptmization.h:346-389) registers
 * each scan against a local map built from its keyframes instead of the cropped prior map:
 * extractSurroundingKeyFrames (:964-978) -> extractNearby (:872-907) or extractForLoopClosure
 * (:857-870) -> extractCloud (:909-955).  The keyframe store mirrors cloudKeyPoses3D/6D and
 * corner/surfCloudKeyFrames; the caller pushes each new key pose + its down-sampled feature clouds
 * (fbr_keyframes_add) and rewrites poses after a loop closure, from its own GTSAM graph
 * (fbr_keyframes_set_pose) or from the pose graph below (fbr_pg_apply).  Selection runs on the host (a few
 * hundred poses), the transforms, concatenation, VoxelGrids and the kNN grid on the device. */
typedef struct fbr_keypose {   /* PointXYZIRPYT (mapOptmization.h:34-51) */
  float x, y, z;
  float intensity;             /* key index: set to the keyframe's position by fbr_keyframes_add,
                                  as saveKeyFramesAndFactor does (:1687, :1694)                   */
  float roll, pitch, yaw;
  float pad_;
  double time;                 /* timeLaserCloudInfoLast when the keyframe was saved (:1698)     */
} fbr_keypose;

typedef struct fbr_keyframe_params {
  float search_radius;         /* surroundingKeyframeSearchRadius 50 m   params.yaml:67        */
  float pose_density;          /* surroundingKeyframeDensity 2 m          params.yaml:66        */
  int32_t loop_closure;        /* loopClosureEnableFlag 0                 params.yaml:70        */
  int32_t submap_size;         /* surroundingKeyframeSize 25              params.yaml:71        */
  double recent_window;        /* 10 s of most recent keyframes           mapOptmization.h:900  */
} fbr_keyframe_params;

void fbr_keyframe_params_default(fbr_keyframe_params* p);
/* cloudKeyPoses3D/6D->push_back + corner/surfCloudKeyFrames.push_back (lidar-frame clouds). */
int fbr_keyframes_add(fbr_ctx* ctx, const fbr_keypose* pose, const fbr_point_xyzi* corner, int64_t n_corner,
                      const fbr_point_xyzi* surf, int64_t n_surf);
/* correctPoses (:1740-1770): new x, y, z, roll, pitch, yaw of keyframe `index` (index and time kept). */
int fbr_keyframes_set_pose(fbr_ctx* ctx, int64_t index, const fbr_keypose* pose);
int fbr_keyframes_count(fbr_ctx* ctx, int64_t* n);
int fbr_keyframes_reset(fbr_ctx* ctx);
/* extractSurroundingKeyFrames at timeLaserCloudInfoLast = `stamp`: the down-sampled local corner /
 * surf maps become the registration map of the following fbr_register / fbr_process_scan calls
 * (registered without the CropBox, as scan2MapOptimization does on them), until fbr_set_map /
 * fbr_load_map restores a prior map.  With no keyframe the previous map is kept (:967-968).
 * n_frames (optional) = entries of cloudToExtract. */
int fbr_extract_surrounding_keyframes(fbr_ctx* ctx, double stamp, const fbr_keyframe_params* kp,
                                      int64_t* n_corner_map, int64_t* n_surf_map, int32_t* n_frames);

/* ---- loop closure (detectLoopClosure / performLoopClosure, mapOptmization.h:606-782) -----------
 * The candidate search runs on the host over the key poses; the clouds, their VoxelGrid and the
 * ICP stay in HBM (the keyframe clouds fbr_keyframes_add stored: no cloud crosses PCIe).
 * fbr_perform_loop_closure returns the between-factor to add: to the pose graph below
 * (fbr_pg_add_loop, fbr_pg_optimize, fbr_pg_apply), or to the caller's own GTSAM graph, which then
 * rewrites the key poses with fbr_keyframes_set_pose.  The loop calls
 * change no key pose and touch neither the registration map, its grids nor a keyframe local map.
 *
 * detectLoopClosure (:606-674) at timeLaserCloudInfoLast = `stamp`:
 *   - radius search around the last key pose with fbr_extract_surrounding_keyframes' conventions:
 *     d2 = ((dx dx + dy dy) + dz dz) in float, accepted when d2 < r^2, ascending d2, ties by index;
 *   - the candidate is the first hit with |time - stamp| > search_time_diff: the nearest
 *     old-enough keyframe (the reference's comment says the oldest; its code takes the nearest);
 *   - no candidate when no hit qualifies or the candidate is the last keyframe itself;
 *   - source: the last keyframe's corner cloud, then its surf cloud, transformed by its stored pose;
 *   - target: keyframes closest - search_num .. closest + search_num (indices < 0 or > latest
 *     skipped), each its corner then its surf cloud under its stored pose, concatenated in that
 *     order, then one VoxelGrid at icp_leaf_size.
 *
 * ICP: pcl::IterativeClosestPoint with TransformationEstimationSVD and DefaultConvergenceCriteria,
 * no rejectors, guess = identity, restated (not pinned against PCL itself, like the oracle):
 *   X = source; final = I; prev_mse = DBL_MAX; it = 0
 *   loop:
 *     for each X[i]: j = nearest target point, d2 = ((dx dx + dy dy) + dz dz) in float, ties to
 *          the lowest target index; a correspondence iff d2 <= max_correspondence_distance^2
 *          (the square taken in double); non-finite points have none
 *     fewer than 3 correspondences: converged = 0, FBR_ICP_NO_CORRESPONDENCES, stop
 *     T = Umeyama without scaling over the correspondences in double (means, sigma = sum (t - mt)
 *         (s - ms)^T / n, SVD sigma = U diag(w) V^T, S = diag(1, 1, det(U) det(V) < 0 ? -1 : 1),
 *         R = U S V^T, t = mt - R ms), rounded to float.  R is always a proper rotation
 *         (det R = +1), for planar and collinear correspondences too, where the sign of
 *         det(sigma) would be rounding noise; for full-rank sigma the two signs agree
 *     X[i] = T X[i] in float, rows ((r0 x + r1 y) + r2 z) + t; final = T final in float; ++it
 *     it >= max_iterations: converged = 1, FBR_ICP_ITERATIONS, stop
 *     cos = 0.5 (T00 + T11 + T22 - 1), t2 = |t|^2 in double; cos >= 1 - transformation_epsilon and
 *         t2 <= transformation_epsilon: converged = 1, FBR_ICP_TRANSFORM, stop
 *     mse = mean d2 of the correspondences (double); |mse - prev_mse| < 1e-12: FBR_ICP_ABS_MSE,
 *         stop; |mse - prev_mse| / prev_mse < euclidean_fitness_epsilon: FBR_ICP_REL_MSE, stop
 *         (both converged = 1); prev_mse = mse
 *   fitness = mean over the source points of the d2 of final * source[i] to its nearest target
 *         point (no distance gate; DBL_MAX when no point has one)
 * Two calls on the same input return the same bytes. */
typedef struct fbr_icp_params {        /* performLoopClosure's "ICP Settings", :689-694 */
  float   max_correspondence_distance; /* 100                                          */
  int32_t max_iterations;              /* 100                                          */
  double  transformation_epsilon;      /* 1e-6                                         */
  double  euclidean_fitness_epsilon;   /* 1e-6                                         */
} fbr_icp_params;

typedef struct fbr_loop_params {
  float   search_radius;      /* historyKeyframeSearchRadius   15   params.yaml:72 */
  float   search_time_diff;   /* historyKeyframeSearchTimeDiff 30 s params.yaml:73 */
  int32_t search_num;         /* historyKeyframeSearchNum      25   params.yaml:74 */
  float   fitness_score;      /* historyKeyframeFitnessScore   0.3  params.yaml:75 */
  float   icp_leaf_size;      /* downSizeFilterICP leaf; 0 = the ctx's mapping_surf_leaf_size (:192) */
  fbr_icp_params icp;
} fbr_loop_params;

/* fbr_icp_result.convergence */
#define FBR_ICP_NOT_CONVERGED 0
#define FBR_ICP_ITERATIONS 1
#define FBR_ICP_TRANSFORM 2
#define FBR_ICP_ABS_MSE 3
#define FBR_ICP_REL_MSE 4
#define FBR_ICP_NO_CORRESPONDENCES 5

typedef struct fbr_icp_result {
  int32_t converged;          /* icp.hasConverged()                                      */
  int32_t convergence;        /* FBR_ICP_*                                               */
  int32_t iterations;         /* nr_iterations_                                          */
  int32_t n_correspondences;  /* of the last iteration                                   */
  double  fitness;            /* icp.getFitnessScore()                                   */
  float   transform[16];      /* icp.getFinalTransformation(), row-major                 */
} fbr_icp_result;

/* fbr_loop_result.status */
#define FBR_LOOP_CLOSED 0
#define FBR_LOOP_NO_CANDIDATE 1      /* detectLoopClosure returned false                  */
#define FBR_LOOP_NOT_CONVERGED 2     /* :715 first half                                   */
#define FBR_LOOP_REJECTED_FITNESS 3  /* :715 second half                                  */

typedef struct fbr_loop_result {
  int32_t status;
  int32_t latest_id, closest_id;     /* -1 when there is no candidate                     */
  int32_t n_source, n_target;        /* latestKeyFrameCloud / DS'd nearHistoryKeyFrameCloud sizes */
  fbr_icp_result icp;
  float   pose_corrected[6];         /* tCorrect = correction * tWrong (:739-741), [r,p,y,x,y,z] */
  float   pose_closest[6];           /* poseTo (:744)                                     */
  float   between[16];               /* poseFrom.between(poseTo) = tCorrect^-1 * tClosest, row-major, computed in double */
} fbr_loop_result;

void fbr_loop_params_default(fbr_loop_params* p);
/* detectLoopClosure alone: FBR_OK with both ids -1 when there is no candidate (no keyframes
 * included). */
int fbr_detect_loop_closure(fbr_ctx* ctx, double stamp, const fbr_loop_params* lp, int32_t* latest_id,
                            int32_t* closest_id);
/* performLoopClosure up to the factor (:676-758).  With FBR_LOOP_NO_CANDIDATE the ids are -1 and the
 * remaining fields zero; otherwise every field is filled, whatever the status (pose_corrected and
 * between are what the reference would have used had it accepted the match). */
int fbr_perform_loop_closure(fbr_ctx* ctx, double stamp, const fbr_loop_params* lp, fbr_loop_result* out);
/* The ICP above on two host clouds (the search grid's cells follow the ctx's mapping_surf_leaf_size). */
int fbr_icp_align(fbr_ctx* ctx, const fbr_point_xyzi* source, int64_t n_source, const fbr_point_xyzi* target,
                  int64_t n_target, const fbr_icp_params* ip, fbr_icp_result* out);
/* Diagnostic: the ICP correspondence search alone (tests compare with a brute-force host search).
 * index[i] = the nearest target point of query[i] with d2 <= max_distance^2, d2[i] its float squared
 * distance; index -1 (and d2 = FLT_MAX) when there is none. */
int fbr_selftest_nn1(fbr_ctx* ctx, const fbr_point_xyzi* target, int64_t n_target, const fbr_point_xyzi* query,
                     int64_t n_query, float max_distance, int32_t* index, float* d2);

/* ---- loop closure for many keyframe pairs (DESIGN §4.8 "many pairs") ---------------------------
 * The calls above close one loop, for the last keyframe.  The ones below take an explicit list of
 * pairs (to re-close a recorded session, or to re-check loops after fbr_pg_apply moved the key
 * poses) and advance the ICP of all pairs of a chunk in the same kernel launches.  Every result is
 * byte for byte what the single call returns for that pair; two calls return the same bytes, and
 * so do different chunk sizes and pair orders. */
typedef struct fbr_loop_pair {
  int32_t latest_id, closest_id;  /* 0 <= closest_id, latest_id < keyframe count, closest_id != latest_id */
  int32_t use_guess;              /* 1: pose_guess stands for latest_id's stored pose, exactly as
                                     match.pose_guess does in fbr_perform_loop_closure_sc */
  float   pose_guess[6];
  int32_t reserved_;
} fbr_loop_pair;

/* detectLoopClosure's rule for every keyframe i >= first_keyframe in ascending order, as it stood
 * when i was the last keyframe: the search runs over keyframes 0..i with stamp = keyframe i's time
 * (the float d2 < r^2 test, ascending d2 with ties by index), takes the first hit with
 * |time - stamp| > search_time_diff, and none if that hit is i itself.  At most one pair per
 * keyframe, use_guess = 0.  Host only.  cap too small: FBR_ERR_CAPACITY with *n_pairs the needed
 * count (pairs == NULL with cap == 0 is the size query); the first cap pairs are written. */
int fbr_loop_candidates(fbr_ctx* ctx, const fbr_loop_params* lp, int32_t first_keyframe, fbr_loop_pair* pairs,
                        int64_t cap, int64_t* n_pairs);
/* out[p] is performLoopClosure for pairs[p] with latest_id as the last keyframe: the target window
 * closest_id +- search_num is clipped to [0, latest_id]; source, target, VoxelGrid, ICP, status,
 * pose_corrected and between as fbr_perform_loop_closure's.  With latest_id the last keyframe it is
 * that call's result; for an earlier keyframe it is what that call returned when latest_id was the
 * last keyframe with the same stored poses.  An invalid pair: FBR_ERR_INVALID_ARG before anything
 * is enqueued.  n_pairs == 0: FBR_OK.  No key pose, registration map or keyframe local map is
 * touched.  chunk_pairs: pairs in flight at once; 0 = as many as the library's device-byte budget
 * allows (csrc/fbr_knobs.h loop_batch_bytes).  No result depends on it. */
int fbr_perform_loop_closures(fbr_ctx* ctx, const fbr_loop_params* lp, const fbr_loop_pair* pairs, int64_t n_pairs,
                              int32_t chunk_pairs, fbr_loop_result* out /* [n_pairs] */);
/* fbr_icp_align per pair on host clouds, the ICPs of a chunk in the same launches. */
int fbr_icp_align_batch(fbr_ctx* ctx, const fbr_point_xyzi* const* sources, const int64_t* n_sources,
                        const fbr_point_xyzi* const* targets, const int64_t* n_targets, int64_t n_pairs,
                        const fbr_icp_params* ip, int32_t chunk_pairs, fbr_icp_result* out /* [n_pairs] */);

/* ---- place recognition: scan-context descriptors and search ---------------------
 * The registration path needs a pose guess near the truth, and fbr_detect_loop_closure needs the
 * last keyframe's stored pose within search_radius of the place it revisits.  The calls below find
 * the place from the clouds alone: every keyframe's lidar-frame corner + surf cloud (already in HBM,
 * fbr_keyframes_add) gets a Scan Context descriptor (Kim & Kim, IROS 2018), and a query is compared
 * with every stored descriptor at every column shift on the device: the exact minimum, no ring-key
 * shortlist, no shift window.
 *
 * This is the project's own restatement of Scan Context.  It is not pinned against any
 * third-party code (neither the authors' nor SC-LIO-SAM's), and the reference has no counterpart.
 *
 * Descriptor D[n_ring][n_sector] (float) of a cloud, in float, operation by operation
 * (csrc/fbr_sc.h, compiled for the device and for the CPU probe of the tests; no FMA contraction):
 *   r      = sqrt(x * x + y * y), correctly rounded
 *   a point counts iff x, y, z are finite and r < max_radius (r == max_radius is dropped; the
 *          largest float below max_radius lands in the last ring)
 *   ring   = min(n_ring - 1, (int)floorf((r / max_radius) * (float)n_ring))
 *   theta  = atan2f(y, x) (glibc's, csrc/fbr_fdlibm.h); if (theta < 0) theta = theta + (float)(2 pi)
 *          (x > 0, y = +-0: theta = 0, sector 0; x < 0, y = +0 or -0: theta = +pi or -pi + 2 pi,
 *          both sector n_sector / 2 for an even n_sector)
 *   sector = min(n_sector - 1, (int)floorf((theta / (float)(2 pi)) * (float)n_sector))
 *   D[ring][sector] = the maximum of max(z + lidar_height, 0) over the cell's points; an empty
 *          cell is 0.
 * The descriptor does not depend on the order of the points.  A keyframe's descriptor is built
 * from its corner cloud followed by its surf cloud.
 *
 * Distance of a query Q to a candidate C at shift s in [0, n_sector):
 *   columns c = 0 .. n_sector - 1 ascending; norm(X, c) = sqrt of the double sum over the rings
 *   (ascending) of X[r][c]^2; a column counts only where norm(Q, c) > 0 and norm(C, (c + s) mod
 *   n_sector) > 0; cos_c = (sum_r Q[r][c] C[r][(c + s) mod n_sector]) / (norm(Q, c) norm(C, (c + s)
 *   mod n_sector)), sums in double with the rings ascending (the device multiplies by the two inverse
 *   norms, a difference of a few double ulps); d(s) = 1 - (sum_c cos_c) / n_eff, or 1.0 when no
 *   column counts.
 *   A candidate's match is min_s d(s), ties to the lowest shift; candidates rank by (distance,
 *   keyframe index) ascending.
 *
 * Pose hypothesis of a match: delta = (float)(shift * 2 pi / n_sector) (the product in double),
 *   pose_guess = fbr_pose_from_affine(fbr_affine_from_pose(stored pose of the keyframe) *
 *   fbr_affine_from_pose({0, 0, delta, 0, 0, 0})) with the float product of the loop closure's
 *   tCorrect: the sensor at the keyframe's position, turned about its own z by delta.  A scan taken
 *   at a keyframe's position with its yaw increased by delta matches at shift ~ delta n_sector / 2 pi.
 *
 * Two calls on the same input return the same bytes (integer maxima, fixed summation orders, no
 * float or double atomics).
 *
 * dist_threshold: the default 0.2 lies between the true matches (<= 0.17) and the nearest false
 * ones (>= 0.23) seen on the project's synthetic fixtures.  It has not been measured on real data. */
typedef struct fbr_sc_params {
  int32_t n_ring;        /* 20, 1..32 */
  int32_t n_sector;      /* 60, 2..64 */
  float max_radius;      /* 80 m */
  float lidar_height;    /* 2.0 m, added to z so that ground returns are positive */
  float dist_threshold;  /* loop acceptance; default 0.2 (see above) */
  int32_t reserved_[3];
} fbr_sc_params;

typedef struct fbr_sc_match {
  int32_t keyframe, shift;   /* keyframe -1: no candidate */
  double distance;
  float pose_guess[6];       /* [roll, pitch, yaw, x, y, z] */
  float pad_[2];
} fbr_sc_match;

#define FBR_SC_MAX_K 16

void fbr_sc_params_default(fbr_sc_params* p);
/* Diagnostic, and the query's first half: the descriptor of a host cloud (corner then surf), built
 * on the device.  desc_out [n_ring * n_sector], ring-major. */
int fbr_sc_describe(fbr_ctx* ctx, const fbr_sc_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, float* desc_out);
/* Describes the keyframes added since the last call (one launch for all of them); *n_described
 * (optional) = how many.  A descriptor depends only on the lidar-frame cloud: fbr_keyframes_set_pose
 * invalidates nothing.  fbr_keyframes_reset, or a call with another n_ring, n_sector, max_radius or
 * lidar_height, discards the store (the next update describes every keyframe).  The query and loop
 * calls below run it themselves. */
int fbr_sc_update(fbr_ctx* ctx, const fbr_sc_params* sp, int64_t* n_described);
/* Diagnostic: the stored descriptor of one keyframe (shape: the last fbr_sc_update's).
 * FBR_ERR_STATE when that keyframe has not been described yet. */
int fbr_sc_descriptor(fbr_ctx* ctx, int64_t keyframe, float* desc_out);
/* The query cloud in the form the keyframes hold: mapping-leaf down-sampled corner and surf features
 * in the lidar frame.  Searches every keyframe; out[0 .. *n_out) = the min(k, N) best matches in
 * rank order, whatever their distance (dist_threshold is not applied); *n_out = 0 without keyframes.
 * 1 <= k <= FBR_SC_MAX_K.  Invalid parameters: FBR_ERR_INVALID_ARG before anything is enqueued.  One
 * device-to-host copy (the N candidate records); the host never touches a descriptor. */
int fbr_sc_query(fbr_ctx* ctx, const fbr_sc_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                 const fbr_point_xyzi* surf, int64_t n_surf, int k, fbr_sc_match* out, int* n_out);
/* detectLoopClosure by appearance: the query is the last keyframe's stored descriptor, the
 * candidates every other keyframe with |time - stamp| > lp->search_time_diff (fbr_detect_loop_closure's
 * expression).  The best candidate is returned if its distance is below dist_threshold; otherwise
 * both ids are -1 (FBR_OK).  *match (optional) = the best candidate either way (keyframe -1 and
 * zeros when there is no candidate at all). */
int fbr_sc_detect_loop_closure(fbr_ctx* ctx, double stamp, const fbr_loop_params* lp, const fbr_sc_params* sp,
                               int32_t* latest_id, int32_t* closest_id, fbr_sc_match* match);
/* fbr_perform_loop_closure with two substitutions for this call only: the candidate comes from
 * fbr_sc_detect_loop_closure, and match.pose_guess stands for the stored pose of the last keyframe
 * wherever performLoopClosure reads it (the source cloud's transform, tWrong, and through them
 * pose_corrected and between).  Every other step, field and status is fbr_perform_loop_closure's (a
 * target range closest +- search_num that reaches the last keyframe itself takes it at its stored
 * pose).  No key pose is changed; the registration map, its grids and a keyframe local map are not
 * touched. */
int fbr_perform_loop_closure_sc(fbr_ctx* ctx, double stamp, const fbr_loop_params* lp, const fbr_sc_params* sp,
                                fbr_loop_result* out, fbr_sc_match* match);

/* ---- pose scoring: one scan against the registration map at many poses -------------
 * How well a scan fits the map at a pose, as a number, for thousands of poses in one launch: the
 * quality figure fbr_reg_stats lacks, and the way to use a coarse seed (a GPS fix, an old pose, a
 * place match a metre off) from which fbr_register converges to nothing.  fbr_pose_search scores a
 * lattice of hypotheses around the seeds; the caller registers from the few best.
 *
 * The score of a pose [roll, pitch, yaw, x, y, z] against the installed map (fbr_set_map,
 * fbr_load_map, fbr_global_map_install); the clouds are taken as given, in the scan frame (callers
 * pass the mapping-leaf down-samples, as for fbr_sc_query):
 *   T = rows 0-2 of fbr_affine_from_pose(pose); q = T p as pointAssociateToMap writes it, float,
 *   ((T0 px + T1 py) + T2 pz) + T3 per coordinate, every step rounded, no contraction.
 *   A corner point searches the corner map, a surf point the surf map.  use_crop = 1: only the map
 *   points inside registration's inclusive box [(-h) + t, h + t] (float, h = fbr_params.crop_half,
 *   t = the pose's translation) count, what fbr_register from that pose would see; use_crop = 0 (and
 *   a keyframe local map, which registration does not crop): the whole map.
 *   d2 = float, flann::L2_Simple's order: d = dx dx; d += dy dy; d += dz dz.  The correspondence of
 *   q is the smallest key (bits(d2) << 32) | map index over those points, so the lowest map index
 *   among equal distances; the point is an inlier iff d2 < g2 = fl(gate * gate).  A non-finite q, or
 *   one with no such point in reach, has no correspondence.
 *   n[k] = the class's points (0 corner, 1 surf), n_in[k] its inliers, sum_d2[k] the inliers' d2,
 *   each widened to double;
 *   fitness = ((sum_d2[0] + sum_d2[1]) + (n_total - n_in_total) * (double)g2) / n_total in double,
 *   DBL_MAX when n_total = 0: a truncated mean, so that a pose with three good matches cannot beat
 *   one with three thousand.
 * 0 < gate <= 1 (the map grid's cell window covers a 1 m radius, the reach the Gauss-Newton search
 * relies on); anything else, a negative pose_chunk or use_crop outside {0, 1}: FBR_ERR_INVALID_ARG.
 *
 * The bytes of a pose's record depend on the pose, the clouds and the map alone: not on the run, on
 * the other poses of the call or on pose_chunk (a fixed summation tree per block of 256 points, the
 * blocks added in order, no float or double atomics).  Poses are processed pose_chunk at a time, so
 * the context's scratch does not grow with n_poses.  Neither call changes the map, the keyframe
 * store or the stream state. */
typedef struct fbr_score_params {
  float gate;          /* 1.0 m */
  int32_t use_crop;    /* 1 */
  int32_t pose_chunk;  /* poses per launch; 0 = 1024 */
  int32_t reserved_[5];
} fbr_score_params;

typedef struct fbr_pose_score {
  int32_t n[2];      /* corner, surf points */
  int32_t n_in[2];   /* ... of them inliers */
  double sum_d2[2];
  double fitness;
} fbr_pose_score;

typedef struct fbr_pose_lattice {
  float half[4];  /* x, y, z (m), yaw (rad): the offsets reach +- half ... */
  float step[4];  /* ... in multiples of step */
} fbr_pose_lattice;

#define FBR_POSE_SEARCH_MAX ((int64_t)1 << 20)  /* hypotheses of one fbr_pose_search */

void fbr_score_params_default(fbr_score_params* p);
/* scores_out [n_poses]; nn_keys_out (optional, tests and diagnostics): [n_poses][n_corner + n_surf],
 * corner points first, the correspondence key of every inlier and ~0 for the other points.  Null
 * or negative arguments: FBR_ERR_INVALID_ARG; no installed map: FBR_ERR_STATE; n_poses = 0 succeeds
 * and writes nothing. */
int fbr_score_poses(fbr_ctx* ctx, const fbr_score_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, const float* poses, int64_t n_poses,
                    fbr_pose_score* scores_out, uint64_t* nn_keys_out);
/* Scores the lattice of hypotheses around n_seeds seed poses [n_seeds][6] and returns the
 * min(top_k, hypotheses) best.  The hypotheses are generated on the host: per axis the offsets are
 * i * step (float) for |i| <= floorf(half / step) (float division); an axis with step = 0 or
 * half = 0 has the single offset 0.  x, y, z are added to the seed's translation and yaw to its yaw,
 * in float.  Order: seed-major, then yaw, z, y, x with x fastest, every axis ascending.  More than
 * FBR_POSE_SEARCH_MAX hypotheses, a negative or non-finite half or step: FBR_ERR_INVALID_ARG.  All
 * hypotheses are scored; the top_k smallest by (fitness, hypothesis index) are returned ascending:
 * poses_out [top_k][6], scores_out [top_k] (optional), index_out [top_k] (optional: the hypothesis
 * indices), *n_out = how many.  Errors as fbr_score_poses; n_seeds = 0 or top_k = 0: *n_out = 0. */
int fbr_pose_search(fbr_ctx* ctx, const fbr_score_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, const float* seeds, int64_t n_seeds,
                    const fbr_pose_lattice* lattice, int64_t top_k, float* poses_out, fbr_pose_score* scores_out,
                    int64_t* index_out, int64_t* n_out);

/* ---- registration information: Hessian and covariance of a registered pose ----------
 * fbr_score_poses says how well a scan fits the map at a pose; this says how well the map determines
 * the pose, and in which directions: the Gauss-Newton normal matrix at the pose, its spectrum, and a
 * covariance in the pose graph's chart, so that fbr_pg_add_between_poses can be given variances that
 * know a corridor from a crossing.  fbr_reg_stats.degenerate (one bit, iteration 0, one threshold)
 * stays what it is.
 *
 * Inputs: a pose p = [roll, pitch, yaw, x, y, z] (float) and corner and surf clouds taken as given,
 * in the scan frame (callers pass the mapping-leaf down-samples, as for fbr_score_poses).  The map is
 * the current registration map; an installed map is cropped by registration's inclusive box
 * [(-h) + t, h + t] (float, h = fbr_params.crop_half, t = p's translation), a keyframe local map is
 * not cropped, as in fbr_register.
 *
 * One pass of cornerOptimization / surfOptimization runs at p exactly as the Gauss-Newton residual
 * pass runs it:
 *   T, trig = pcl::getTransformation of p in float (glibc sinf / cosf), q = T s as
 *   pointAssociateToMap writes it for each scan point s (float, ((T0 sx + T1 sy) + T2 sz) + T3);
 *   the 5 nearest map points of q (corner points in the corner map, surf points in the surf map) by
 *   (d2, map index), d2 in flann::L2_Simple's float order, kept iff d2[4] < 1;
 *   the line fit and its eigenvalue gate (D1[0] > 3 D1[1]) or the plane fit and its 0.2 m gate, then
 *   the residual with s = 1 - 0.9 |d| (corner) or 1 - 0.9 |d| / sqrt(|q|) (surf), kept iff s > 0.1;
 *   the row a = [d/droll, d/dpitch, d/dyaw, c.x, c.y, c.z] and b = -c.intensity, as float32
 *   (LMOptimization, mapOptmization.h:1286-1332).
 * No fit cache and no reuse flag: every query is fitted from its current neighbours.
 *
 * From the accepted rows, in double (a float x float product is exact in double):
 *   H = sum a a^T (the 21 upper entries summed, stored as a full symmetric row-major [36]),
 *   g = sum a b, rss = sum b b; n_rows[2] the accepted rows and n_query[2] the points, corner then surf;
 *   n = n_rows[0] + n_rows[1];  sigma2 = rss / max(n - 6, 1), replaced by params.sigma2 when that is > 0;
 *   eig[6] ascending and evec[36] (row i = the unit eigenvector of eig[i]) by a cyclic Jacobi of H in
 *   double (csrc/fbr_reg_info.h: at most 16 sweeps of the 15 rotations (0,1), (0,2) .. (4,5); rotation
 *   t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq); equal
 *   eigenvalues keep their order of appearance on the diagonal; a sweep that finds every
 *   off-diagonal entry zero ends it; from the fifth sweep on an entry with |a_pp| + 100 |a_pq| == |a_pp|
 *   and |a_qq| + 100 |a_pq| == |a_qq| is set to zero without a rotation);
 *   rank = the number of eig[i] > params.eig_floor (default 100, the reference's degeneracy
 *   threshold, :1359);
 *   cov = sum_i v_i v_i^T w_i,  w_i = sigma2 / eig[i] when eig[i] > eig_floor, otherwise
 *   params.unobserved_variance.  Its default, 1e4, means "unknown": a direction the scan does not
 *   constrain gets a variance no consumer can mistake for a measurement.  (A pseudo-inverse would
 *   report zero variance in exactly that direction, so it is not used.)
 *   cov_tangent = S cov S^T, var_tangent = diag(cov_tangent): S = blockdiag(E, R^T) maps a pose
 *   increment [droll, dpitch, dyaw, dx, dy, dz] to the pose graph's chart T (+) [w; v] =
 *   (R Exp(w), t + R v) (below, "Chart"), R = Rz(yaw) Ry(pitch) Rx(roll),
 *   E = [[1, 0, -sin pitch], [0, cos roll, sin roll cos pitch], [0, -sin roll, cos roll cos pitch]],
 *   both in double from the float pose.  var_tangent is in the order fbr_pg_add_between_poses takes.
 *   flags: FBR_INFO_NO_ROWS (n = 0), FBR_INFO_FEW_ROWS (0 < n < 6), FBR_INFO_BAD_POSE (a non-finite
 *   pose component), FBR_INFO_NOT_REGISTERED (fbr_batch_info: the job did not register).  A flagged
 *   record has H = g = 0, rss = sigma2 = 0, eig = 0, evec = I, rank = 0 and cov = cov_tangent =
 *   unobserved_variance I; n_query and n_rows are still the counts of the pass (0 where no pass ran).
 * eig_floor, unobserved_variance not finite or not > 0, sigma2 negative or not finite, a negative
 * pose_chunk: FBR_ERR_INVALID_ARG.
 *
 * A record's bytes depend on the pose, the clouds and the map alone: not on the other poses of a
 * call, the other jobs of a batch, pose_chunk or the run (one partial per block of 256 queries with
 * a fixed summation tree, a job's partials added in order, no float or double atomics).  Nor do they
 * depend on the order of a cloud's points: each cloud is summed in canonical order, its points sorted
 * ascending by the bit patterns of (x, y, z, intensity) read as unsigned words, so the Morton-ordered
 * down-sample of a batch job and fbr_voxel_grid's key-ordered one of the same features give the same
 * record. */
#define FBR_INFO_NO_ROWS 1
#define FBR_INFO_FEW_ROWS 2
#define FBR_INFO_BAD_POSE 4
#define FBR_INFO_NOT_REGISTERED 8

typedef struct fbr_info_params {
  double eig_floor;            /* 100 */
  double unobserved_variance;  /* 1e4: "unknown" */
  double sigma2;               /* 0: from the residuals */
  int32_t pose_chunk;          /* poses (jobs) per launch; 0 = 1024 */
  int32_t reserved_[5];
} fbr_info_params;

typedef struct fbr_reg_info {
  double H[36];
  double g[6];
  double rss, sigma2;
  double eig[6];
  double evec[36];
  double cov[36];
  double cov_tangent[36];
  double var_tangent[6];
  int32_t n_rows[2];   /* corner, surf rows accepted */
  int32_t n_query[2];  /* corner, surf points */
  int32_t rank;
  int32_t flags;       /* FBR_INFO_* */
} fbr_reg_info;

void fbr_info_params_default(fbr_info_params* p);
/* out [n_poses]; poses [n_poses][6].  Poses are processed pose_chunk at a time on scratch of the
 * call's own, so the context's memory does not grow with n_poses.  Changes neither the map, the
 * stream state, a staged batch nor what fbr_diag_knn_last / fbr_diag_gn_last return.  Null or
 * negative arguments: FBR_ERR_INVALID_ARG; no map: FBR_ERR_STATE; n_poses = 0 succeeds and writes
 * nothing.  A non-finite pose is not an error: its record is flagged. */
int fbr_reg_info_poses(fbr_ctx* ctx, const fbr_info_params* ip, const fbr_point_xyzi* corner, int64_t n_corner,
                       const fbr_point_xyzi* surf, int64_t n_surf, const float* poses, int64_t n_poses,
                       fbr_reg_info* out);
/* The same pass for every job of the latest batch launch, over that launch's down-sampled clouds at
 * each job's result pose (what fbr_batch_results returns): out [n_jobs].  Waits for the launches in
 * flight, as fbr_batch_labels; alters nothing of the launch chain or its results.  A job that did not
 * register (FBR_REG_NOT_ENOUGH_FEATURES, FBR_REG_FEATURE_CAPACITY) gets a flagged record
 * (FBR_INFO_NOT_REGISTERED).  FBR_ERR_STATE before any launch and after a single-scan call has
 * dropped the batch. */
int fbr_batch_info(fbr_ctx* ctx, const fbr_info_params* ip, fbr_reg_info* out /* [n_jobs] */);
/* variances_out[k] = max(info->var_tangent[k], floor[k]) (floor may be NULL: no floor), the noise
 * input of fbr_pg_add_between_poses.  Host only. */
int fbr_reg_info_variances(const fbr_reg_info* info, const double floor[6], double variances_out[6]);

/* ---- pose graph: key poses from odometry, loop and GPS factors ----------------------
 * The reference's addOdomFactor (:1517-1541), addGPSFactor (:1543-1634), the loop BetweenFactor
 * (:743-758) and correctPoses (:1735-1770), as a batch optimiser over the keyframe store, so that
 * "loop closed" can end in corrected key poses without GTSAM.  This is the project's own
 * restatement: it is pinned by a NumPy model in tests/ and not against GTSAM or iSAM2.  What stays
 * with the caller: iSAM2's incremental updates, IMU preintegration factors and robust GPS or odometry
 * factors (robust loop factors are below: "robust loop factors").
 * The marginal covariances of the key poses (poseCovariance, :1706) and addGPSFactor's covariance
 * gate (:1561) are below ("marginal covariances").
 *
 * Nodes 0 .. N-1 are the keyframes in the store when fbr_pg_optimize is called; node i starts from
 * the stored key pose i.  A pose is (R, t), R = Rz(yaw) Ry(pitch) Rx(roll) as fbr_affine_from_pose;
 * all optimiser arithmetic is double (csrc/fbr_pg.h, compiled for the device and for the CPU probe
 * of the tests; no FMA contraction).
 *
 * Chart: GTSAM 4.0's default for Pose3 (no GTSAM_POSE3_EXPMAP):
 *   retraction  T (+) [w; v]  = (R Exp(w), t + R v)
 *   Local(A, B)               = [Log(A_R^T B_R); A_R^T (B_t - A_t)]
 *   tangent order [rotation; translation], the reference's noise vectors (roll, pitch, yaw, x, y, z).
 *
 * Factors; each carries variances and its residual is whitened by 1 / sqrt(variance):
 *   prior(i, Z, var[6])       e = Local(Z, T_i)             PriorFactor<Pose3>, :1523-1525
 *   between(i, j, Z, var[6])  e = Local(Z, T_i^-1 T_j)      BetweenFactor<Pose3>, :1531-1537, :758
 *   gps(i, z, var[3])         e = T_i.t - z                 gtsam::GPSFactor, :1627
 * Cost F = 1/2 sum_k |e_k / sigma_k|^2.
 *
 * Jacobians, analytic, with respect to the chart.  With D = T_i^-1 T_j, E = Z^-1 D, phi = Log(E_R):
 *   d e_rot / d w_j = Jr^-1(phi)              d e_t / d v_j = E_R
 *   d e_rot / d w_i = -Jr^-1(phi) D_R^T       d e_t / d w_i = Z_R^T [D_t]x      d e_t / d v_i = -Z_R^T
 *   Jr^-1(phi) = I + [phi]x / 2 + (1 / t^2 - (1 + cos t) / (2 t sin t)) [phi]x^2, t = |phi| (the
 *   series 1/12 + t^2/720 below t = 1e-3; the second term evaluated as cot(t / 2) / (2 t))
 *   prior: the j half with E = Z^-1 T_i;  gps: d e / d v = R_i, d e / d w = 0.
 *   Log: t = atan2(|vee(R - R^T)| / 2, (trace - 1) / 2); the axis from vee(R - R^T) while
 *   cos t > -0.99, from the symmetric part of R near pi; the series below t = 1e-6.  No NaN at 0 or pi.
 *
 * Method: Levenberg-Marquardt on H = J^T J, g = J^T r.
 *   step:   (H + lambda diag(H)) delta = -g
 *   accept when the cost falls: lambda /= lambda_factor; otherwise lambda *= lambda_factor, retry
 *   FBR_PG_CONVERGED   an accepted step's relative cost decrease < rel_cost_tol or its absolute
 *                      decrease < abs_cost_tol; also a graph whose initial cost is exactly 0 (0 iterations)
 *   FBR_PG_ITERATIONS  max_iterations accepted steps
 *   FBR_PG_STALLED     lambda > lambda_max; the best poses so far are kept
 *   FBR_PG_NUMERICAL   a Cholesky pivot of the solve was non-positive or non-finite (or the initial
 *                      cost is not finite); the optimised poses equal the initial ones
 *   FBR_PG_EMPTY       no keyframes
 * The linear solve splits H = T + L: T, block-tridiagonal in 6x6 blocks, holds every prior, every
 * gps factor, every between factor with |i - j| = 1 and the damping; L every other between factor
 * (the loops).  Conjugate gradients preconditioned by an exact solve with T (block cyclic
 * reduction): one iteration without loops, and with K loops T^-1 H is the identity plus a term of
 * rank <= 6 K.  It stops when r^T M^-1 r <= pcg_rel_tol^2 r0^T M^-1 r0 or after max_pcg_iterations;
 * the iterate is then used as it is (the accept test covers an inexact step).
 * The result is defined by the minimiser, not by the path to it.
 *
 * Output: double [N][6] = [roll, pitch, yaw, x, y, z] with roll = atan2(R21, R22), pitch =
 * asin(-R20) clamped, yaw = atan2(R10, R00); fbr_pg_apply rounds them to float.
 *
 * Two calls on the same store and factors return the same bytes: no float or double atomics, every
 * sum is taken in a fixed order.
 *
 * Robust loop factors (robust != FBR_PG_ROBUST_NONE; opt-in, the default changes nothing).  They
 * apply to the loop factors only: the between factors with |i - j| != 1, the terms of L, where a
 * false place-recognition match arrives.  Priors, odometry and GPS factors are never re-weighted.
 * With s = |r|^2 of a loop factor's whitened residual, e = sqrt(s) and k = robust_scale:
 *   Huber   w = 1 if e <= k, else k / e          rho = s / 2 if e <= k, else k (e - k / 2)
 *   Cauchy  w = 1 / (1 + s / k^2)                rho = (k^2 / 2) log1p(s / k^2)
 * The cost is F = sum rho, with rho = s / 2 for every other factor.  A loop factor is linearised as
 * sqrt(w) r, sqrt(w) J (w = 2 rho'(s) at the linearisation point), which is how GTSAM's
 * noiseModel::Robust whitens.  The accept test, cost_initial, cost_final and the convergence
 * tolerances all use this F.  A robust cost is NOT convex: the result is the local minimiser that
 * Levenberg-Marquardt reaches from the stored poses, and a different start may end elsewhere.
 * Huber with k = 1.345 and Cauchy with k = 3 are reasonable scales; a Cauchy scale near 1 also
 * down-weights true loops when the drift is large.  fbr_pg_loop_weights reports s and w per loop
 * factor, so that a caller can drop rejected loops before fbr_pg_apply and fbr_global_map_build.
 *
 * Direct solve (solver = FBR_PG_SOLVER_DIRECT; opt-in).  With K loop factors, U [6K x 6N] their
 * whitened Jacobians and T the damped block-tridiagonal part, H + lambda diag(H) = T + U^T U and the
 * step is Woodbury's, exact up to rounding whatever K:
 *   y = T^-1 (-g),  W = T^-1 U^T,  C = I + U W = Lc Lc^T,  delta = y - W (Lc Lc^T)^-1 U y.
 * T^-1 by the block cyclic reduction, W and C as the marginal covariances below build them (here on
 * the damped T, once per trial), then one dense forward and backward substitution.  It needs device
 * work space for W (6N x 6K doubles), the solve's chunk of right-hand sides per level, C and z; a need
 * above max_work_mb returns FBR_ERR_CAPACITY before anything is allocated.  pcg_iterations is 0.  A
 * bad pivot of T or of C ends the call with FBR_PG_NUMERICAL.  Choose it when the graph has more
 * than a few loops: the conjugate gradients need up to 6 K + 1 iterations per solve and end at
 * max_pcg_iterations beyond that.  Without loops the step is y and no W or C exists.  Same bytes
 * from two calls, as above. */
typedef struct fbr_pg_params {
  int32_t max_iterations;      /* 30 accepted LM steps */
  int32_t max_pcg_iterations;  /* 200 */
  double rel_cost_tol;         /* 1e-5, GTSAM's relativeErrorTol */
  double abs_cost_tol;         /* 1e-5, GTSAM's absoluteErrorTol */
  double pcg_rel_tol;          /* 1e-8 */
  double lambda_init;          /* 1e-5 */
  double lambda_factor;        /* 10 */
  double lambda_max;           /* 1e10 */
  int32_t solver;              /* FBR_PG_SOLVER_PCG 0 (the default) | FBR_PG_SOLVER_DIRECT 1 */
  int32_t robust;              /* FBR_PG_ROBUST_NONE 0 (the default) | FBR_PG_ROBUST_HUBER 1 | FBR_PG_ROBUST_CAUCHY 2 */
  float robust_scale;          /* k, in units of the whitened residual's norm; > 0 and finite when robust != 0 */
  int32_t max_work_mb;         /* the direct solver's device work-space bound; 0 = 2048 */
} fbr_pg_params;

#define FBR_PG_SOLVER_PCG 0
#define FBR_PG_SOLVER_DIRECT 1
#define FBR_PG_ROBUST_NONE 0
#define FBR_PG_ROBUST_HUBER 1
#define FBR_PG_ROBUST_CAUCHY 2

/* fbr_pg_result.status */
#define FBR_PG_CONVERGED 0
#define FBR_PG_ITERATIONS 1
#define FBR_PG_STALLED 2
#define FBR_PG_NUMERICAL 3
#define FBR_PG_EMPTY 4

typedef struct fbr_pg_result {
  int32_t status;              /* FBR_PG_* */
  int32_t iterations;          /* accepted LM steps */
  int32_t trials;              /* accepted and rejected */
  int32_t pcg_iterations;      /* total */
  int32_t n_nodes;
  int32_t n_factors;
  int32_t n_loop_factors;      /* factors in L */
  int32_t pad_;
  double cost_initial;
  double cost_final;
  double lambda;
  double max_translation_change;  /* over the nodes, optimised against stored */
  double max_rotation_change;
} fbr_pg_result;

void fbr_pg_params_default(fbr_pg_params* p);
/* Empties the factor list (fbr_keyframes_reset does the same). */
int fbr_pg_reset(fbr_ctx* ctx);
/* Factors.  Node indices must name existing keyframes, variances must be finite and > 0, measurements
 * finite, i != j: otherwise FBR_ERR_INVALID_ARG and nothing is stored.  `between` is row-major, as
 * fbr_loop_result.between, and is taken as it is (its rotation block is not re-orthonormalised). */
int fbr_pg_add_prior(fbr_ctx* ctx, int64_t node, const float pose[6], const double variances[6]);
int fbr_pg_add_between(fbr_ctx* ctx, int64_t i, int64_t j, const float between[16], const double variances[6]);
/* poseFrom.between(poseTo) computed in double: odometry is added this way (:1533-1537). */
int fbr_pg_add_between_poses(fbr_ctx* ctx, int64_t i, int64_t j, const float pose_i[6], const float pose_j[6],
                             const double variances[6]);
int fbr_pg_add_gps(fbr_ctx* ctx, int64_t node, const double xyz[3], const double variances[3]);
/* With r->status == FBR_LOOP_CLOSED: the between factor (latest_id, closest_id, r->between,
 * (float)r->icp.fitness x 6) of :746-758, *added (optional) = 1; otherwise nothing, *added = 0. */
int fbr_pg_add_loop(fbr_ctx* ctx, const fbr_loop_result* r, int* added);
int fbr_pg_factor_count(fbr_ctx* ctx, int64_t* n);
/* Optimises the key poses under the factors.  Changes no key pose, no map and no grid.  A node that
 * no factor touches: FBR_ERR_STATE.  A graph without a prior is allowed (the damping makes it
 * solvable).  One host read per Levenberg-Marquardt trial; the conjugate-gradient iterations are
 * enqueued ahead of a host-mapped progress word, as the ICP's. */
int fbr_pg_optimize(fbr_ctx* ctx, const fbr_pg_params* p, fbr_pg_result* out);
/* The last optimise's poses; *n = their count.  FBR_ERR_STATE without a result, FBR_ERR_CAPACITY
 * (with *n set) if cap < *n. */
int fbr_pg_poses(fbr_ctx* ctx, double* poses_out /* [n][6] */, int64_t cap, int64_t* n);
/* Every loop factor in add order at the last optimise's final poses: its index in the factor list,
 * s = |r|^2 of its whitened residual and its weight w (1 with robust = FBR_PG_ROBUST_NONE, which makes
 * the call a plain chi-square report).  The values are the device's, of the evaluation at the result
 * poses.  *n = their count.  Errors as fbr_pg_poses. */
int fbr_pg_loop_weights(fbr_ctx* ctx, int32_t* factor_index_out, double* chi2_out, double* weight_out, int64_t cap,
                        int64_t* n);
/* correctPoses (:1735-1770): every key pose gets its optimised x, y, z, roll, pitch, yaw rounded to
 * float through fbr_keyframes_set_pose (index and time kept).  FBR_ERR_STATE when there is no result
 * or the store has changed size since the optimise. */
int fbr_pg_apply(fbr_ctx* ctx);

/* ---- pose graph: marginal covariances of the key poses and the GPS gate -------------
 * The reference reads poseCovariance = isam->marginalCovariance(last) after every update (:1706) and
 * adds a GPS factor only while poseCovariance(3,3) or (4,4) is at least poseCovThreshold (:1561).
 *
 * Definition: Sigma = H^-1, H = J^T J the UNDAMPED normal matrix (lambda = 0) of every factor in the
 * list, linearised at the last optimise's poses exactly as fbr_pg_poses returns them (the double
 * Euler angles, converted back by R = Rz(yaw) Ry(pitch) Rx(roll)), so that a model reproduces the
 * point from public outputs.  After a robust optimise (fbr_pg_params.robust) the loop factors carry
 * their weights at those poses, with that optimise's kind and scale: H is that of the weighted
 * Jacobians sqrt(w) J, so that a rejected false loop does not shrink the covariances at full
 * weight; with robust = 0 nothing changes.  The marginal of node i is the 6x6 diagonal block Sigma_ii, row-major,
 * in the chart's tangent order [rotation; translation]; the translation part is in the body frame
 * of T_i, as GTSAM's Pose3 marginal is; entries (3,3) and (4,4) are what the reference reads.  The
 * output is exactly symmetric: r <= c is computed and mirrored.
 *
 * Method: H = T0 + U^T U, T0 the undamped block-tridiagonal part and U [6K x 6N] the K loop factors'
 * whitened Jacobians (two 6x6 blocks per block row).  Sigma_ii = P_i - Y_i^T Y_i with
 *   P_i = (T0^-1)_ii,  W = T0^-1 U^T,  C = I + U W = Lc Lc^T,  Y = Lc^-1 W^T.
 * P_i by selected inversion through the levels of the optimiser's block cyclic reduction of T0:
 * walking up from the last level with P[m] = S[m][m] and Q[m] = S[m][m-1] per node (S the level's
 * inverse).  Last level: P[0] = D^-1.  Even node m = 2q: P[m] = next.P[q].  Odd node k, a = (k-1)/2,
 * Sl = next.P[a], Sr = next.P[a+1], Srl = next.Q[a+1], G_k = D_k^-1 T[k][k-1], H_k = D_k^-1 T[k][k+1]:
 *   S[k][k-1] = -G_k Sl - H_k Srl          S[k][k+1] = -G_k Srl^T - H_k Sr
 *   P[k] = D_k^-1 - S[k][k-1] G_k^T - S[k][k+1] H_k^T     Q[k] = S[k][k-1]     Q[k+1] = S[k][k+1]^T
 * (terms of an absent right neighbour dropped).  W by one cyclic-reduction solve per column, rhs_chunk
 * columns per pass; C by a dense blocked Cholesky (panels of 32 columns).
 *
 * T0 must be positive definite: an unbroken chain of consecutive between factors and at least one
 * prior or gps factor.  A non-positive or non-finite pivot of T0 or of C: status FBR_PG_NUMERICAL and
 * a zeroed output (return value FBR_OK).  Under the reference's prior (variance 1e8 on the
 * translation) cond(H) ~ 1e16 and the covariances carry two to three digits: enough for the gate,
 * whose two sides are orders of magnitude apart.
 *
 * FBR_ERR_STATE without an optimise result, or when the store's size or the factor count has changed
 * since that optimise.  FBR_ERR_INVALID_ARG for a node index out of range.  FBR_ERR_CAPACITY (with
 * out->n_out set) when cap < the rows asked for, and (with out->work_bytes set) when the device
 * work space, W (6N x 6K doubles) plus P, Q, the chunk's right-hand sides, C and the output, exceeds
 * max_work_bytes.  Two calls return the same bytes, whatever rhs_chunk and whichever nodes are asked
 * for: no float or double atomics, every sum in a fixed order.  One device-to-host copy of the result
 * and one read of the status word per call; nothing waits in between. */
typedef struct fbr_pg_marginal_params {
  int32_t rhs_chunk;       /* columns of U^T solved per pass; 0 = default (48) */
  int32_t reserved_[3];
  int64_t max_work_bytes;  /* 0 = default (2 GiB) */
} fbr_pg_marginal_params;
typedef struct fbr_pg_marginal_result {
  int32_t status;          /* FBR_PG_CONVERGED (ok) | FBR_PG_NUMERICAL | FBR_PG_EMPTY (no row asked for) */
  int32_t n_nodes, n_loop_factors, n_out;
  int64_t work_bytes;
} fbr_pg_marginal_result;
void fbr_pg_marginal_params_default(fbr_pg_marginal_params* p);
/* nodes == NULL: every node in order (n_nodes ignored, cap = rows of cov_out).  A node may be named
 * more than once. */
int fbr_pg_marginals(fbr_ctx* ctx, const fbr_pg_marginal_params* p, const int64_t* nodes, int64_t n_nodes,
                     double* cov_out /* [n][36] */, int64_t cap, fbr_pg_marginal_result* out);
/* addGPSFactor's gate (:1561) on the last node: *wanted = !(cov33 < thr && cov44 < thr); cov_xy
 * (optional) = {cov33, cov44}.  Without a covariance (FBR_PG_NUMERICAL) the factor is wanted and
 * cov_xy is infinite.  Errors as fbr_pg_marginals. */
int fbr_pg_gps_gate(fbr_ctx* ctx, double pose_cov_threshold, int* wanted, double cov_xy[2]);

/* ---- global map (visualizeGlobalMapThread's save block, mapOptmization.h:485-521) -------------
 * Turns the keyframe store into the map the localiser loads: every keyframe's corner / surf cloud
 * transformed by its current key pose (fbr_affine_from_pose on the host, then
 * ((T0 x + T1 y) + T2 z) + T3 per row, as fbr_extract_surrounding_keyframes), concatenated in
 * keyframe order, and filtered by downSizeFilterCorner / downSizeFilterSurf.  Everything happens in
 * HBM on the clouds fbr_keyframes_add stored; the result stays in device buffers of the context
 * until the next build, fbr_keyframes_reset or fbr_destroy.  A build changes neither the
 * registration map, nor its grids, nor any key pose.
 *
 * Points with a non-finite coordinate after the transform are dropped (the reference leaves the
 * case undefined) and counted in n_dropped; they belong to neither the filtered nor the raw clouds.
 *
 * Reference mode (wide = 0, the default): pcl::VoxelGrid's semantics, the filter every other
 * entry point uses (exact_voxel_order applies).  PCL gives up when its cell count
 * dx * dy * dz exceeds INT32_MAX ("Leaf size is too small") and returns its input: the cloud is
 * then the unfiltered concatenation and *_overflow is set.  At the 0.2 m corner leaf that limit is
 * roughly a 250 m cube, which any real trajectory exceeds.
 *
 * Wide mode (wide = 1) is this project's own extension, not the reference's behaviour: where PCL
 * would overflow, the cloud is filtered by a VoxelGrid with 64-bit keys; where it would not, by the
 * normal filter (the two modes then return the same bytes).  The wide filter:
 *   - inv, min_b, max_b, div_b and ijk exactly as PCL's: the float min / max box and
 *     ijk = (int)(floorf(p * inv) - (float)min_b);
 *   - key = ijk0 + ijk1 * div0 + ijk2 * div0 * div1 in uint64; voxels in ascending key order;
 *   - centroid = the float sum of x, y, z, intensity over the voxel's points in input index order,
 *     divided by the float count; exact_voxel_order has no meaning here (PCL has no order to
 *     reproduce on overflow) and is ignored;
 *   - FBR_ERR_CAPACITY when div0 * div1 * div2 >= 2^63, when some |bound * inv| >= 2^24
 *     (floorf(p * inv) stops being an exact cell number) or for more than INT32_MAX points;
 *   - no float atomics: two calls return the same bytes. */
typedef struct fbr_gmap_params {
  float corner_leaf, surf_leaf;   /* <= 0: fbr_params.mapping_corner_leaf_size / mapping_surf_leaf_size */
  int32_t wide;                   /* 0 (default): PCL semantics, overflow -> output = input;
                                     1: the wide filter where PCL would overflow, the normal path otherwise */
  int32_t keep_raw;               /* keep the unfiltered concatenations (cloudGlobal.pcd) */
  int32_t reserved_[4];
} fbr_gmap_params;

typedef struct fbr_gmap_result {
  int64_t n_keyframes, n_corner_raw, n_surf_raw, n_corner, n_surf, n_dropped;
  int32_t corner_overflow, surf_overflow;   /* PCL's overflow condition held */
  int32_t corner_wide, surf_wide;           /* the wide filter produced the cloud */
} fbr_gmap_result;

#define FBR_GMAP_SAVE_GLOBAL 1  /* fbr_global_map_save: also cloudGlobal.pcd */

/* corner_leaf = surf_leaf = 0 (the context's mapping leaves), wide = 0, keep_raw = 0. */
void fbr_gmap_params_default(fbr_gmap_params* p);
/* Builds the map from all keyframes in index order (params NULL: the defaults; result optional).
 * n_*_raw count the concatenations' points after the drop.  With no keyframes: FBR_OK, all counts 0
 * (an empty map is built). */
int fbr_global_map_build(fbr_ctx* ctx, const fbr_gmap_params* params, fbr_gmap_result* result);
/* The built clouds (sizes, then optional copies; pass NULL to skip), as fbr_get_map.
 * FBR_ERR_STATE when no build has been done. */
int fbr_global_map_get(fbr_ctx* ctx, int64_t* n_corner, int64_t* n_surf, fbr_point_xyzi* corner,
                       fbr_point_xyzi* surf);
/* Exactly what fbr_set_map does on the built clouds: the start-up VoxelGrid at the
 * context's mapping leaves, the kNN grids, registration with the CropBox.  The built clouds are
 * filtered and gridded where they are (no cloud is uploaded); fbr_get_map downloads the installed
 * map when it is asked for.  FBR_ERR_STATE when no build has been done. */
int fbr_global_map_install(fbr_ctx* ctx);
/* Writes the reference's files into the existing directory `dir` (:495-519), never removing
 * anything (the reference's `rm -r` of the directory is not reproduced):
 *   cloudCorner.pcd, cloudSurf.pcd   the built clouds (fbr_pcd_write_ascii)
 *   trajectory.pcd                   x, y, z, intensity of the key poses the build used (cloudKeyPoses3D)
 *   transformations.pcd              those key poses (cloudKeyPoses6D, fbr_pcd_write_poses_ascii)
 *   cloudGlobal.pcd                  raw corner then raw surf; only with FBR_GMAP_SAVE_GLOBAL in
 *                                    flags and a build that kept them (keep_raw)
 * FBR_ERR_STATE when no build has been done, FBR_ERR_INVALID_ARG when a file cannot be written. */
int fbr_global_map_save(fbr_ctx* ctx, const char* dir, int32_t flags);
/* pcl::io::savePCDFileASCII of a PointXYZIRPYT cloud (host only): FIELDS x y z intensity roll pitch
 * yaw time, SIZE 4 4 4 4 4 4 4 8, TYPE F F F F F F F F, COUNT 1 each; values by fbr_pcd_write_ascii's
 * rules (8 significant digits, "nan" spelled out), `time` too.  The layout is this project's reading
 * of PCL's field registration for PointXYZIRPYT (mapOptmization.h:34-51); it has not been pinned
 * against PCL's own writer. */
int fbr_pcd_write_poses_ascii(const char* path, const fbr_keypose* keyposes, int64_t n);
/* Test hook: the wide filter alone on a host cloud, whether PCL would overflow on it or not
 * (points with a non-finite coordinate are skipped, as fbr_voxel_grid does).  out holds n points. */
int fbr_selftest_voxel_wide(fbr_ctx* ctx, const fbr_point_xyzi* in, int64_t n, float leaf, fbr_point_xyzi* out,
                            int64_t* n_out);

/* Down-sampled global map actually used (sizes, then optional copies; pass NULL to skip).  After
 * fbr_extract_surrounding_keyframes: the keyframe local map (laserCloud{Corner,Surf}FromMapDS). */
int fbr_get_map(fbr_ctx* ctx, int64_t* n_corner, int64_t* n_surf, fbr_point_xyzi* corner,
                fbr_point_xyzi* surf);

/* A2+A4: projectPointCloud() + cloudExtraction() (imageProjection.cpp:583-670).
 * Fills the cloud_info fields (msg/cloud_info.msg:5-9,32): start_ring/end_ring [n_scan],
 * col_ind/range/cloud [n_out] (size the buffers for n_in points). */
int fbr_project(fbr_ctx* ctx, const fbr_point_xyzirt* points, int64_t n_in, int32_t* start_ring,
                int32_t* end_ring, int32_t* col_ind, float* range, fbr_point_xyzi* cloud,
                int64_t* n_out);

/* A6-A9: FeatureExtraction::featureExtra() on the ctx's last projection
 * (featureExtraction.h:79-294).  label[n_out] gets cloudLabel (1 corner, -1 picked surf, 0);
 * corner/surf get cloud_corner / cloud_surface (size corner for 20*6*n_scan points and surf for
 * n_out points).  Any output pointer may be NULL. */
int fbr_extract_features(fbr_ctx* ctx, int8_t* label, fbr_point_xyzi* corner, int64_t* n_corner,
                         fbr_point_xyzi* surf, int64_t* n_surf);

/* A10-A18: mapOptimization::registration() (mapOptmization.h:263-343) on given feature clouds,
 * ignoring the time gate.  pose_inout: [roll,pitch,yaw,x,y,z] guess in, registered pose out. */
int fbr_register(fbr_ctx* ctx, const fbr_point_xyzi* corner, int64_t n_corner,
                 const fbr_point_xyzi* surf, int64_t n_surf, float pose_inout[6],
                 fbr_reg_stats* stats);
/* Same, also returning the pose after every Gauss-Newton iteration (trace [max_iterations][6]). */
int fbr_register_trace(fbr_ctx* ctx, const fbr_point_xyzi* corner, int64_t n_corner,
                       const fbr_point_xyzi* surf, int64_t n_surf, float pose_inout[6],
                       fbr_reg_stats* stats, float* trace);

/* One scan through the whole path in stream mode (cloudHandler after the cache queue,
 * imageProjection.cpp:197-225): the FeatureExtraction scratch state carries over between calls
 * as in the reference; `stamp` feeds the mappingProcessInterval gate (mapOptmization.h:279).
 * Returns as soon as the pose is known (the Gauss-Newton solve that ends the run writes it to
 * host-mapped memory); Gauss-Newton iterations enqueued ahead of that point may still be draining
 * on the context's stream, and every other entry point waits for them first.  The caller's buffer
 * may be reused once the call returns. */
int fbr_process_scan(fbr_ctx* ctx, const fbr_point_xyzirt* points, int64_t n_in, double stamp,
                     float pose_inout[6], fbr_reg_stats* stats);
/* Forget the carried FeatureExtraction / time-gate state (as a freshly constructed node). */
int fbr_reset_stream(fbr_ctx* ctx);

/* Independent jobs (config C4): each job is one scan registered from its own guess against the
 * shared map, with fresh FeatureExtraction state.  Processed in device batches of max_batch; the
 * host scans are packed into pinned staging and copied on a second stream, double-buffered, so
 * batch k+1's host-to-device copy overlaps batch k's compute.  The caller's buffers may be reused
 * once the call returns. */
int fbr_process_batch(fbr_ctx* ctx, const fbr_point_xyzirt* const* scans, const int64_t* n_in,
                      int n_jobs, float* poses_inout /* [n_jobs][6] */,
                      fbr_reg_stats* stats /* [n_jobs] or NULL */);
/* Diagnostic: the kNN grid of the current map: {sparse (hashed chunks) 0/1, surf-grid box dims
 * x, y, z, box cells, stored chunks (sparse) or cells (dense), corner points, surf points}. */
int fbr_map_grid_info(fbr_ctx* ctx, int64_t info[8]);
/* Host-to-device scan bytes copied by the last fbr_process_batch (ingest measurement). */
int fbr_ingest_bytes(fbr_ctx* ctx, double* h2d_bytes);
/* Diagnostic process-wide counters: kernel launches, blocking host synchronisations of the
 * boundary code, and host polls of the device Gauss-Newton flags; reset != 0 zeroes them. */
int fbr_debug_counters(long long* launches, long long* host_syncs, long long* flag_polls, int reset);

/* Device-resident batch (throughput measurement): stage copies the scans and guesses to HBM (and
 * computes the per-job CropBox map statistics, which depend only on the guesses); launch enqueues
 * the whole path for the staged batch (asynchronous, inputs are not modified so it may be
 * re-launched); wait blocks; results copies the latest launch's poses/stats out.
 * Launches are pipelined fbr_params.pipeline_depth deep (1..3, default 3; 1 when max_batch = 1):
 * consecutive launches rotate over the work buffers and streams of the launch slots, and
 * fbr_batch_launch returns once the launch two before it is fully enqueued, leaving the tail of its own Gauss-Newton loop (whose length the device decides)
 * to the next launch / flush / wait call.  So launch n's projection and features run beside launch
 * n-1's last iterations.  The single-scan entry points (fbr_project, fbr_register*,
 * fbr_process_scan) share the device buffers and drop a staged batch (after enqueueing every
 * launch in flight): fbr_batch_launch then returns FBR_ERR_STATE until the next fbr_batch_stage.
 * Without deskew tables and field-timed motions the staged scans live on the device as 16-B
 * records (x, y, z, ring): intensity and time reach no batch result (poses, statistics, feature
 * masks) and are not copied; a batch staged that way and then given deskew tables (fbr_set_deskew)
 * or FBR_TIME_FIELD motions (fbr_set_motion) is reported FBR_ERR_STATE at launch (stage it again).
 * FBR_TIME_COLUMN motions read no time and run on the records. */
int fbr_batch_stage(fbr_ctx* ctx, const fbr_point_xyzirt* const* scans, const int64_t* n_in,
                    int n_jobs, const float* poses_in /* [n_jobs][6] */);
int fbr_batch_launch(fbr_ctx* ctx);
/* Enqueue the rest of every launch in flight (host side only; no device synchronisation). */
int fbr_batch_flush(fbr_ctx* ctx);
int fbr_batch_wait(fbr_ctx* ctx);
/* A job whose features exceeded the device capacity (k_features' window / segment limits) does not
 * fail the batch: it gets status FBR_REG_FEATURE_CAPACITY and its guess as pose, and the others
 * their results (fbr_batch_results, fbr_process_batch). */
int fbr_batch_results(fbr_ctx* ctx, float* poses_out /* [n_jobs][6] */,
                      fbr_reg_stats* stats /* [n_jobs] or NULL */);
/* Whole feature masks for batch jobs (featureExtraction.h:178-285, cloudLabel).  By default a batch
 * resolves each segment's surf walk only within reach of its end, the only picks that reach a pose
 * or a statistic, so its label masks are incomplete.  With on != 0, the following fbr_batch_launch
 * calls run every walk whole (as fbr_extract_features does), at some cost in throughput; results
 * are the same either way. */
int fbr_batch_set_full_masks(fbr_ctx* ctx, int on);
/* cloudLabel of job `job` of the latest launch (1 corner, -1 picked surf, 0), one entry per
 * projected point: *n_out = the job's point count (cloud_info order).  FBR_ERR_STATE unless that
 * launch ran with full masks; FBR_ERR_CAPACITY (with *n_out set) if cap < *n_out.  Waits for the
 * launches in flight. */
int fbr_batch_labels(fbr_ctx* ctx, int job, int8_t* label, int64_t cap, int64_t* n_out);
/* Diagnostic (A/B and tests).  A batch launch staged from 16-B records, without deskew and with the
 * default-order four-wave ring filter, keeps its projected cloud as 12-B (x, y, z) records; every
 * other launch keeps 16-B float4.  Results are the same either way.  force_wide 1: the following
 * launches keep float4; 0: the default; < 0: the switch is left as it is.  *point_bytes (may be
 * NULL) receives the record size of the latest batch launch's cloud: 12, 16, or 0 before any. */
int fbr_diag_batch_cloud(fbr_ctx* ctx, int force_wide, int32_t* point_bytes);
/* Diagnostic (tests): the last neighbour search of the latest single-scan registration on this
 * context (fbr_register, fbr_register_trace, fbr_process_scan), i.e. the pass of its last
 * LMOptimization call, which ran at the pose before that call's step.  *n_corner / *n_surf: the
 * down-sampled query counts (stats n_corner_ds / n_surf_ds).  Per query, corner queries first, each
 * in its cloud's order: queries[3 i ..] the map-frame position the pass searched from (float, its
 * bits), nbr[5 i ..] the five map indices (positions in fbr_get_map's clouds) in (d2, index) order,
 * or -1 five times when the search kept no correspondence.  *desc (may be NULL) names the kernel
 * that ran the pass.  cap = 0 returns the counts and the descriptor only; FBR_ERR_CAPACITY when
 * 0 < cap < *n_corner + *n_surf; FBR_ERR_STATE when the context's latest registration was not a
 * single scan (none yet, or a batch launch since). */
typedef struct fbr_knn_desc {
  int32_t iterations; /* LMOptimization calls of the run; the pass read back is number iterations - 1 */
  int32_t r, rx;      /* grid cells per side covering 1 m along y / z and along x */
  int32_t flat;       /* 1: flat LDS row queue */
  int32_t sparse;     /* 1: hashed-chunk grids */
  int32_t lpq;        /* lanes per query (1 or 8) */
  int32_t fused;      /* 1: fused with the residual (tail mode) */
  int32_t tiles;      /* 1: LDS block tiles (with the grid search behind them) */
} fbr_knn_desc;
int fbr_diag_knn_last(fbr_ctx* ctx, int32_t* n_corner, int32_t* n_surf, float* queries /* [cap][3] */,
                      int32_t* nbr /* [cap][5] */, int64_t cap, fbr_knn_desc* desc);
/* Diagnostic (tests): the residual pass that followed that search, under the same preconditions.
 * Per query, in fbr_diag_knn_last's order: points[3 i ..] the down-sampled scan-frame point the
 * query was transformed from, fit_state (0 none, 1 fitted, 2 rejected by the eigenvalue
 * / plane gate) and fit[6 i ..] of the query's fit cache (corner: two line points; surf: pa, pb, pc,
 * pd and two unused floats), nsame 1 where the search found the previous pass's five neighbours and
 * the cached fit was reused (-1 for every query when the pass ran fused with the search, which keeps
 * no such flag).  Per work item of the job: items[4 k ..] = {job, 0 corner / 1 surf, first query,
 * queries} and partial[32 k ..] its normal-equation partial (21 upper AtA entries, 6 AtB, the row
 * count, 4 zero pads).  T_trig (may be NULL): T[12] and trig[6] the pass ran at.  cap = 0 and
 * item_cap = 0 return the counts only; FBR_ERR_CAPACITY when a non-zero capacity is too small. */
int fbr_diag_gn_last(fbr_ctx* ctx, int32_t* n_corner, int32_t* n_surf, float* points /* [cap][3] */,
                     int8_t* fit_state /* [cap] */, float* fit /* [cap][6] */, int8_t* nsame /* [cap] */, int64_t cap,
                     int32_t* n_items,
                     int32_t* items /* [item_cap][4] */, double* partial /* [item_cap][32] */, int64_t item_cap,
                     float* T_trig /* [18] */);
/* Enqueue (on the ctx stream, after every launch in flight) a copy of the latest launch's per-job
 * pose records {pose[6] f32, iterations i32, status i32} = 32 B/job into `device_dst` (device
 * memory of the ctx's device, [n_jobs][8] x 4 B) — the payload of the cross-GPU pose all-gather. */
int fbr_batch_export(fbr_ctx* ctx, void* device_dst);
/* Pipelined form: export the records of the oldest launch not yet exported, if it is fully
 * enqueued (after fbr_batch_launch n: at least launch n - (pipeline_depth - 1); after fbr_batch_flush:
 * every launch), without waiting for the launches in flight; launches are exported in launch
 * order, each once.  The copy runs on that launch's stream after it, and after the
 * work queued so far on `wait_stream` (a HIP stream of the caller still reading device_dst, or
 * NULL); *export_stream receives the stream to wait on before reading device_dst, *launch_id the
 * launch number (0, 1, ... since the context was created), or -1 (nothing to export: no copy). */
int fbr_batch_export_ready(fbr_ctx* ctx, void* device_dst, void* wait_stream, void** export_stream,
                           int64_t* launch_id);
/* ---- multi-GPU pose gather ---------------------------------------------------
 * Scans shard across the GPUs of a node: one process (and one ctx) per GPU, each registering its
 * own contiguous block of jobs against its replica of the map; nothing is exchanged on the data
 * path.  The only collective is the all-gather of the 32-B pose records {pose[6] f32, iterations
 * i32, status i32} over RCCL (xGMI), after each launch.  librccl is loaded on the first call
 * (FBR_ERR_UNSUPPORTED if it cannot be); a one-GPU host never needs it.
 *   rank 0:     fbr_comm_unique_id(id), then hands id to the other ranks (any out-of-band channel);
 *   every rank: fbr_comm_create(&comm, ctx, id, nranks, rank, max_jobs_per_rank)  (blocks until
 *               all ranks joined), then per launch fbr_batch_allgather(ctx, comm, launch_id, recv,
 *               wait_stream, &stream) with the same launch_id on every rank.
 * max_jobs_per_rank must be at least the ctx's fbr_params.max_batch (FBR_ERR_CAPACITY otherwise), so
 * no staged batch can exceed the communicator's blocks once it exists. */
#define FBR_COMM_ID_BYTES 128
typedef struct fbr_comm fbr_comm;
int fbr_comm_unique_id(uint8_t id_out[FBR_COMM_ID_BYTES]);
int fbr_comm_create(fbr_comm** out, fbr_ctx* ctx, const uint8_t id[FBR_COMM_ID_BYTES], int nranks, int rank,
                    int max_jobs_per_rank);
/* One process driving several devices (one host thread, one ctx and one rank per device, SURVEY §7
 * step 7): the communicators of all n contexts at once, rank i = ctxs[i] (distinct devices), made
 * with one RCCL unique id inside an ncclGroupStart / ncclGroupEnd.  Each thread then calls
 * fbr_batch_allgather with its own ctx and out[i], the same launch ids on every thread; each
 * communicator is destroyed with fbr_comm_destroy. */
int fbr_comm_create_local(fbr_comm** out /* [n] */, fbr_ctx* const* ctxs, int n, int max_jobs_per_rank);
int fbr_comm_destroy(fbr_comm* comm);
/* Collective (every rank, same launch_id; -1 = the latest launch): the records of that launch of
 * every rank into recv = [nranks][max_jobs_per_rank][8] x 4 B (device memory of the ctx's device;
 * rank r's block holds its staged jobs in order, then zero records).  Records follow
 * fbr_batch_results (a job over the feature capacity: its guess, FBR_REG_FEATURE_CAPACITY).  The
 * launch is first enqueued to its end (the host follows its GN flags); the export and the
 * all-gather then run on that launch's stream, returned in *done_stream (wait on it before reading
 * recv), or, with done_stream NULL, joined into the ctx stream.  Consecutive calls are ordered on
 * the device (each after the previous one's all-gather).  recv is written only after the work
 * queued so far on `wait_stream` (a HIP stream of the caller still reading the previous result out
 * of recv, or NULL when recv is read only on *done_stream / the ctx stream), so one recv buffer may
 * serve every call.
 * The launch must still own its work slot (one of the last pipeline_depth launches of the staged
 * batch): FBR_ERR_STATE otherwise.  Every argument and state check runs before anything is
 * enqueued, but the call is a collective: a rank that returns an error has not joined the
 * all-gather, its peers stay blocked in it, and the caller must tear the group down (every rank:
 * fbr_comm_destroy, which aborts the RCCL communicator after a failed call). */
int fbr_batch_allgather(fbr_ctx* ctx, fbr_comm* comm, int64_t launch_id, void* recv, void* wait_stream,
                        void** done_stream);

/* Sum of the per-scan algorithmic byte counts of the last completed batch (roofline input). */
int fbr_batch_bytes(fbr_ctx* ctx, double* bytes_total, double* bytes_gn);

/* Kernel timing with HIP events recorded on the ctx stream around every launch of the named
 * kernel ("gn_residual", "project", ...). */
int fbr_set_profiling(fbr_ctx* ctx, int enable);
/* Restrict the timing to a comma-separated list of kernel names (NULL or "" = all kernels). */
int fbr_set_profiling_kernels(fbr_ctx* ctx, const char* names);
int fbr_kernel_time(fbr_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);
void* fbr_stream(fbr_ctx* ctx);

/* VoxelGrid<PointXYZI>::filter on the device (the kernel every DS in the path uses). */
int fbr_voxel_grid(fbr_ctx* ctx, const fbr_point_xyzi* in, int64_t n, float leaf,
                   fbr_point_xyzi* out, int64_t* n_out);

/* Diagnostic: device numerics probe.  For i < n writes out[6i..6i+5] = {sqrtf(|a|), a/b,
 * atan2f(a,b), a*b+b*a-a, sinf(a), cosf(a)} computed by the device kernels' primitives (tests
 * compare the bits with the host libm the reference uses). */
int fbr_selftest_math(int n, const float* a, const float* b, float* out);

/* Diagnostic: cv::eigen of n symmetric 6x6 float matrices a[36i..36i+35] (the degeneracy step,
 * mapOptmization.h:1353) by the single-lane and the wave-parallel device Jacobi; out[84i..] =
 * {6 eigenvalues, 36 eigenvector entries} of each (tests compare both with the host restatement). */
int fbr_selftest_eigen6(int n, const float* a, float* out);

/* Diagnostic: the per-query functions of the Gauss-Newton residual pass, one lane per case.
 * in[28 i ..] = {kind (0 corner, 1 surf), five neighbours x y z, the map-frame query x y z, the
 * scan-frame point x y z, trig[6]}; out[20 i ..] = {fit ok, fit[6], apply ok, coeff[4], row[6], b,
 * 0}: corner_fit / surf_fit, corner_apply / surf_apply and the LMOptimization row of the product
 * (mapOptmization.h:1016-1211, :1286-1332).  Whatever a rejected stage would have written is 0. */
int fbr_selftest_gn_rows(int n, const float* in, float* out);
/* Diagnostic: the workgroup reduction of the item partials.  Set s holds 256 rows rows[(256 s + t)
 * * 7 ..] = {row[6], b} with flags ok[256 s + t] (a slot whose flag is 0 contributes nothing);
 * out[32 s ..] = the 28 sums (21 upper AtA products, 6 AtB, the count) and 4 zero pads. */
int fbr_selftest_gn_reduce(int n_sets, const float* rows, const int8_t* ok, double* out);
/* Diagnostic: cv::solve(A, b, DECOMP_QR) and Mat::inv (LU) on n 6x6 float systems, one lane each:
 * a[36 i ..], b[6 i ..] -> x[6 i ..] and inv[36 i ..]; ret[2 i ..] = the two return codes (0:
 * singular, the corresponding output is then unspecified). */
int fbr_selftest_solve6(int n, const float* a, const float* b, float* x, float* inv, int32_t* ret);

/* Diagnostic: the degeneracy fast path of the iteration-0 solve.  out[i] = 1 when every eigenvalue
 * of the symmetric 6x6 float matrix a[36i..36i+35] is certified above thr (LDL^T of A - (thr +
 * 1e-3 ||A||_F) I in double), so isDegenerate (mapOptmization.h:1353-1366) is false without the
 * Jacobi; 0 = not certified (the device then runs cv::eigen's Jacobi). */
int fbr_selftest_eig_certified(int n, const float* a, float thr, int32_t* out);

/* Diagnostic: PCL VoxelGrid's point order inside voxels.  perm[0..n) = the index order the device's
 * emulation of std::sort's partition phase (libstdc++ introsort, fbr_introsort.h) leaves the
 * (keys[i], i) pairs in; a stable sort of that sequence by key is std::sort's result.  lds = 1
 * runs the LDS variant of the per-segment kernels (n <= 8192), 2 LDS keys with global-memory
 * positions (the mapping-DS kernel's, n <= 18432), 3 the per-ring filter's shape (512 threads, all
 * in LDS, n <= 4096, whole-workgroup partitions from 128 elements), 0 the global-memory one. */
int fbr_selftest_voxel_order(int64_t n, const uint32_t* keys, int lds, uint32_t* perm);
/* Diagnostic: the VoxelGrid kernels' stable LSD radix sorts on one array of n keys (the low
 * `nbits` significant), one workgroup: variant 0 = the per-ring filter's LDS sort (512 threads,
 * 8-bit digits, n <= 4096), 1 = the per-segment LDS sort (256 threads, 9-bit digits, n <= 4096),
 * 2 = the global-scratch sort (1024 threads), 3 = the mapping DS's in-place LDS sort (1024 x 18),
 * 4 = variant 3 with ballot-leader digit counts, 5 = variant 4 with round 3's wave-uniform early
 * exits in its count and scatter loops (the exact form round 3 reverted), 6 = the in-place sort
 * of the mapping DS's small size class (256 x 16, n <= 4096).  keys_inout receives
 * the sorted keys, perm the source index of every sorted position. */
int fbr_selftest_radix_sort(int64_t n, int nbits, int variant, uint32_t* keys_inout, uint32_t* perm);

/* Measurement helper: achievable HBM bandwidth of a device-wide float4 copy of `bytes` (read +
 * write counted), averaged over `iters` launches (the STREAM-copy figure bench.py reports next to
 * the 8 TB/s spec peak). */
int fbr_stream_copy_bandwidth(int hip_device, int64_t bytes, int iters, double* gbps);
/* Measurement helper: the VALU issue roof.  Every SIMD holds waves_per_simd (1..8) waves, each lane
 * running 8 independent chains of one VALU instruction (kind 0 v_fma_f32, 1 v_add_u32, 2
 * v_pk_fma_f32) for 32 * iters instructions; *ginst_per_s = wave-level instructions per second over
 * `reps` launches, *ms_per_launch (optional) the launch time (tools/valu_calib.py). */
int fbr_valu_peak(int hip_device, int waves_per_simd, int kind, int iters, int reps, double* ginst_per_s,
                  double* ms_per_launch);

/* pcl::getTransformation / pcl::getTranslationAndEulerAngles (row-major 4x4 float). */
void fbr_affine_from_pose(const float pose[6], float m[16]);
void fbr_pose_from_affine(const float m[16], float pose[6]);

#ifdef __cplusplus
}
#endif
#endif /* FBR_H_ */
