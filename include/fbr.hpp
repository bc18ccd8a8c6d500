/* fbr.hpp — header-only C++ host mirror of the reference's operator interface for the hot path,
 * layered on the C-ABI in fbr.h (libfbr_hip.so).  No ROS, PCL or Eigen types: the cloud_info
 * message is mirrored by fbr::CloudInfo (msg/cloud_info.msg fields on the path) and
 * Eigen::Affine3f by fbr::Affine3f (row-major 4x4 float, Eigen's matrix() element order).
 *
 *   reference (file:line)                                         mirror
 *   ImageProjection::cloudHandler / projectPointCloud /             fbr::ImageProjection::cloudHandler
 *     cloudExtraction (src/imageProjection.cpp:182-226, 583-670)    (+ the static pose chain :206-218)
 *   FeatureExtraction::featureExtra (src/featureExtraction.h:79)    fbr::FeatureExtraction::featureExtra
 *   mapOptimization::registration (src/mapOptmization.h:263-343)    fbr::MapOptimization::registration
 *
 * Error behaviour follows the reference: a scan that fails the cachePointCloud checks is dropped
 * (cloudHandler returns false); too few features leave the pose untouched (status in lastStats()).
 * Device or argument errors, which the reference has no analogue for, throw fbr::Error.
 *
 * The three objects share one fbr::Context (one HIP device + stream), because the device keeps the
 * projection, feature state and map resident between the stages — the reference's objects are
 * also members of one node (imageProjection.cpp:96-97).
 */
#ifndef FBR_HPP_
#define FBR_HPP_

#include <array>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "fbr.h"

namespace fbr {

struct Error : std::runtime_error {
  int status;
  Error(int s, const char* what) : std::runtime_error(std::string(what) + ": " + fbr_strerror(s)), status(s) {}
};

inline void check(int s, const char* what) {
  if (s != FBR_OK) throw Error(s, what);
}

/* Eigen::Affine3f as a row-major 4x4 float matrix. */
struct Affine3f {
  float m[16];
  static Affine3f Identity() {
    Affine3f a{};
    a.m[0] = a.m[5] = a.m[10] = a.m[15] = 1.0f;
    return a;
  }
  /* pcl::getTransformation(x, y, z, roll, pitch, yaw) */
  static Affine3f fromPose(const float rpyxyz[6]) {
    Affine3f a;
    fbr_affine_from_pose(rpyxyz, a.m);
    return a;
  }
  /* pcl::getTranslationAndEulerAngles -> [roll, pitch, yaw, x, y, z] */
  void toPose(float rpyxyz[6]) const { fbr_pose_from_affine(m, rpyxyz); }
  float x() const { return m[3]; }
  float y() const { return m[7]; }
  float z() const { return m[11]; }
};

/* The cloud_info fields the path reads or writes (msg/cloud_info.msg:5-9, 32-34), plus the
 * feature mask (FeatureExtraction::cloudLabel, featureExtraction.h:41). */
struct CloudInfo {
  double stamp = 0.0;                         // header.stamp.toSec()
  std::vector<int32_t> startRingIndex;        // [N_SCAN]
  std::vector<int32_t> endRingIndex;          // [N_SCAN]
  std::vector<int32_t> pointColInd;           // [n]
  std::vector<float> pointRange;              // [n]
  std::vector<fbr_point_xyzi> cloud_deskewed; // [n] extractedCloud
  std::vector<fbr_point_xyzi> cloud_corner;   // cornerCloud (visit order)
  std::vector<fbr_point_xyzi> cloud_surface;  // surfaceCloud (per-ring DS, ring order)
  std::vector<int8_t> cloudLabel;             // [n] 1 corner, -1 picked surf, 0
};

/* One HIP device + stream + device-resident state (RAII over fbr_ctx). */
class Context {
 public:
  explicit Context(const fbr_params& p, int hip_device = 0) : p_(p) {
    check(fbr_create(&ctx_, &p_, hip_device), "fbr_create");
  }
  ~Context() {
    if (ctx_) fbr_destroy(ctx_);
  }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  fbr_ctx* get() const { return ctx_; }
  const fbr_params& params() const { return p_; }

 private:
  fbr_params p_;
  fbr_ctx* ctx_ = nullptr;
};

/* sensor_msgs/PointCloud2 as the node receives it (an owned copy: what cloudQueue holds,
 * imageProjection.cpp:233). */
struct PointCloud2 {
  struct Field {
    std::string name;
    uint32_t offset = 0;
    uint8_t datatype = FBR_PF_FLOAT32;
    uint32_t count = 1;
  };
  double stamp = 0.0;  // header.stamp.toSec()
  uint32_t height = 1, width = 0, point_step = 0, row_step = 0;
  bool is_bigendian = false, is_dense = true;
  std::vector<Field> fields;
  std::vector<uint8_t> data;
};

/* ImageProjection (imageProjection.cpp:29): projectPointCloud + cloudExtraction on the device. */
class ImageProjection {
 public:
  explicit ImageProjection(Context& c) : c_(c) {}
  ImageProjection(const ImageProjection&) = delete;

  /* cloudHandler's projection half (:197-199).  Returns false where cachePointCloud drops the
   * scan (:229-301: a ring outside [0, N_SCAN) is not an error there, only points are skipped;
   * an empty cloud yields an empty CloudInfo). */
  bool cloudHandler(const fbr_point_xyzirt* pts, int64_t n, double stamp, CloudInfo& info) {
    const int H = c_.params().n_scan;
    info.stamp = stamp;
    info.startRingIndex.assign(H, 0);
    info.endRingIndex.assign(H, 0);
    info.pointColInd.resize(n);
    info.pointRange.resize(n);
    info.cloud_deskewed.resize(n);
    int64_t n_out = 0;
    check(fbr_project(c_.get(), pts, n, info.startRingIndex.data(), info.endRingIndex.data(),
                      info.pointColInd.data(), info.pointRange.data(), info.cloud_deskewed.data(), &n_out),
          "fbr_project");
    info.pointColInd.resize(n_out);
    info.pointRange.resize(n_out);
    info.cloud_deskewed.resize(n_out);
    info.cloud_corner.clear();
    info.cloud_surface.clear();
    info.cloudLabel.clear();
    return true;
  }

  /* cachePointCloud (:229-301): the 2-message delay queue; returns false while it fills, else
   * makes the oldest message current (timeScanCur = its stamp). */
  bool cachePointCloud(const PointCloud2& msg) {
    cloudQueue_.push_back(msg);
    if (cloudQueue_.size() <= 2) return false;
    current_ = std::move(cloudQueue_.front());
    cloudQueue_.pop_front();
    return true;
  }

  /* cloudHandler's projection half on a raw message: the cache queue, then the message bytes are
   * unpacked on the device (fromROSMsg), checked (is_dense / ring -> fbr::Error with FBR_ERR_MSG
   * where the reference calls ros::shutdown()), and projected.  msgFlags() reports the warnings
   * (FBR_MSG_NO_TIME: the reference's "deskew function disabled" ROS_WARN). */
  bool cloudHandler(const PointCloud2& msg, CloudInfo& info) {
    if (!cachePointCloud(msg)) return false;
    std::vector<fbr_point_field> f(current_.fields.size());
    for (size_t k = 0; k < f.size(); ++k)
      f[k] = fbr_point_field{current_.fields[k].name.c_str(), current_.fields[k].offset, current_.fields[k].datatype,
                             current_.fields[k].count};
    fbr_pointcloud2 m;
    m.height = current_.height;
    m.width = current_.width;
    m.fields = f.data();
    m.n_fields = (int32_t)f.size();
    m.is_bigendian = current_.is_bigendian;
    m.point_step = current_.point_step;
    m.row_step = current_.row_step;
    m.data = current_.data.data();
    m.data_size = current_.data.size();
    m.is_dense = current_.is_dense;
    const int H = c_.params().n_scan;
    const int64_t n = (int64_t)current_.width * current_.height;
    info.stamp = current_.stamp;
    info.startRingIndex.assign(H, 0);
    info.endRingIndex.assign(H, 0);
    info.pointColInd.resize(n);
    info.pointRange.resize(n);
    info.cloud_deskewed.resize(n);
    int64_t n_out = 0;
    check(fbr_project_msg(c_.get(), &m, info.startRingIndex.data(), info.endRingIndex.data(), info.pointColInd.data(),
                          info.pointRange.data(), info.cloud_deskewed.data(), &n_out, &msg_flags_),
          "fbr_project_msg");
    info.pointColInd.resize(n_out);
    info.pointRange.resize(n_out);
    info.cloud_deskewed.resize(n_out);
    info.cloud_corner.clear();
    info.cloud_surface.clear();
    info.cloudLabel.clear();
    return true;
  }
  int msgFlags() const { return msg_flags_; }

  /* deskewInfo() enabled (imageProjection.cpp:189-191 uncommented): the table fbr_imu_deskew_info
   * built for the next scan; deskewPoint then runs inside the device compaction. */
  void setDeskew(const fbr_deskew_table& t) { check(fbr_set_deskew(c_.get(), &t, 1), "fbr_set_deskew"); }
  void clearDeskew() { check(fbr_set_deskew(c_.get(), nullptr, 0), "fbr_set_deskew"); }

  /* The odometry half of deskewInfo() and findPosition's body enabled: the motion record of the
   * next scan (from odomDeskewInfo or motionFromPoses, its FBR_MOTION_* flags set by the caller). */
  void setMotion(const fbr_motion& m) { check(fbr_set_motion(c_.get(), &m, 1), "fbr_set_motion"); }
  void clearMotion() { check(fbr_set_motion(c_.get(), nullptr, 0), "fbr_set_motion"); }
  /* odomDeskewInfo (imageProjection.cpp:395-491); returns the number of samples to pop. */
  static int64_t odomDeskewInfo(const std::vector<fbr_odom_sample>& queue, double timeScanCur, double timeScanNext,
                                fbr_odom_info& out) {
    int64_t n_pop = 0;
    check(fbr_odom_deskew_info(queue.data(), (int64_t)queue.size(), timeScanCur, timeScanNext, &out, &n_pop),
          "fbr_odom_deskew_info");
    return n_pop;
  }
  /* Constant velocity from the last two registration results, for hosts without odometry. */
  static void motionFromPoses(const float prev[6], const float cur[6], double dt, double scanPeriod, double dtNext,
                              fbr_motion& out, float guessOut[6]) {
    check(fbr_motion_from_poses(prev, cur, dt, scanPeriod, dtNext, &out, guessOut), "fbr_motion_from_poses");
  }
  /* updateInitialGuess (mapOptmization.h:799-855) on a caller-owned state. */
  static void updateInitialGuess(fbr_guess_state& state, const fbr_odom_info* odom, const fbr_deskew_table* table,
                                 bool haveKeyframes, bool useImuHeading, float pose[6]) {
    check(fbr_update_initial_guess(&state, odom, table, haveKeyframes ? 1 : 0, useImuHeading ? 1 : 0, pose),
          "fbr_update_initial_guess");
  }

 private:
  Context& c_;
  std::deque<PointCloud2> cloudQueue_;
  PointCloud2 current_;
  int msg_flags_ = 0;
};

/* FeatureExtraction (featureExtraction.h:19): featureExtra(cloud_info) on the projection the
 * context holds (the same scan ImageProjection just handled). */
class FeatureExtraction {
 public:
  explicit FeatureExtraction(Context& c) : c_(c) {}

  void featureExtra(CloudInfo& info) {
    const int64_t n = (int64_t)info.pointColInd.size();
    const int64_t corner_cap = 20 * 6 * (int64_t)c_.params().n_scan;
    info.cloudLabel.resize(n);
    info.cloud_corner.resize(corner_cap);
    info.cloud_surface.resize(n);
    int64_t nc = 0, ns = 0;
    check(fbr_extract_features(c_.get(), info.cloudLabel.data(), info.cloud_corner.data(), &nc,
                               info.cloud_surface.data(), &ns),
          "fbr_extract_features");
    info.cloud_corner.resize(nc);
    info.cloud_surface.resize(ns);
  }

 private:
  Context& c_;
};

/* mapOptimization (mapOptmization.h:54): prior map + registration(cloud_info, Affine3f&). */
class MapOptimization {
 public:
  explicit MapOptimization(Context& c) : c_(c) {}

  /* corner_GlobalMap / surf_GlobalMap as loaded from the PCDs (:245-260; the start-up VoxelGrid is
   * applied on the device). */
  void setGlobalMap(const std::vector<fbr_point_xyzi>& corner, const std::vector<fbr_point_xyzi>& surf) {
    check(fbr_set_map(c_.get(), corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size()),
          "fbr_set_map");
  }

  /* The start-up block itself (:245-260): loadPCDFile(getenv("HOME") + savePCDDirectory +
   * "cloudCorner.pcd" / "cloudSurf.pcd") then the DS.  Unlike the reference (which ignores
   * loadPCDFile's return value and runs with an empty map), an unreadable file throws. */
  void loadGlobalMap(const std::string& savePCDDirectory) {
    const char* home = std::getenv("HOME");
    const std::string dir = std::string(home ? home : "") + savePCDDirectory;
    loadGlobalMapFiles(dir + "cloudCorner.pcd", dir + "cloudSurf.pcd");
  }
  void loadGlobalMapFiles(const std::string& corner_pcd, const std::string& surf_pcd) {
    check(fbr_load_map(c_.get(), corner_pcd.c_str(), surf_pcd.c_str()), "fbr_load_map");
  }

  /* registration (:263-343): mappingProcessInterval gate, getTranslationAndEulerAngles of the
   * guess, CropBox + DS + scan2MapOptimization on the device, getTransformation of the result. */
  void registration(const CloudInfo& info, Affine3f& pose_guess) {
    stats_ = fbr_reg_stats{};
    if (!(info.stamp - timeLastProcessing_ >= c_.params().mapping_process_interval)) {
      stats_.status = FBR_REG_SKIPPED_INTERVAL;
      return;
    }
    timeLastProcessing_ = info.stamp;
    float pose[6];
    pose_guess.toPose(pose);
    check(fbr_register(c_.get(), info.cloud_corner.data(), (int64_t)info.cloud_corner.size(),
                       info.cloud_surface.data(), (int64_t)info.cloud_surface.size(), pose, &stats_),
          "fbr_register");
    pose_guess = Affine3f::fromPose(pose);
  }

  const fbr_reg_stats& lastStats() const { return stats_; }

  /* LIO-SAM keyframe back-end (mapOptmization.h:857-978, 1667-1770): the caller's GTSAM step pushes
   * each key pose with its DS'd feature clouds and corrects poses after a loop closure;
   * extractSurroundingKeyFrames then makes the keyframe local map the registration map. */
  void addKeyFrame(const fbr_keypose& pose, const std::vector<fbr_point_xyzi>& corner,
                   const std::vector<fbr_point_xyzi>& surf) {
    check(fbr_keyframes_add(c_.get(), &pose, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size()),
          "fbr_keyframes_add");
  }
  void correctPose(int64_t index, const fbr_keypose& pose) {
    check(fbr_keyframes_set_pose(c_.get(), index, &pose), "fbr_keyframes_set_pose");
  }
  void extractSurroundingKeyFrames(double timeLaserCloudInfoLast, const fbr_keyframe_params& kp) {
    check(fbr_extract_surrounding_keyframes(c_.get(), timeLaserCloudInfoLast, &kp, nullptr, nullptr, nullptr),
          "fbr_extract_surrounding_keyframes");
  }

  /* Loop closure (mapOptmization.h:606-782).  detectLoopClosure returns false when there is no
   * candidate; performLoopClosure runs the ICP on the device and returns the fbr_loop_result: with
   * status FBR_LOOP_CLOSED the caller adds BetweenFactor(latest_id, closest_id, between,
   * Variances(icp.fitness)) to its graph and writes the optimised poses back with correctPose. */
  bool detectLoopClosure(double timeLaserCloudInfoLast, const fbr_loop_params& lp, int* latestID, int* closestID) {
    int32_t a = -1, b = -1;
    check(fbr_detect_loop_closure(c_.get(), timeLaserCloudInfoLast, &lp, &a, &b), "fbr_detect_loop_closure");
    if (latestID) *latestID = a;
    if (closestID) *closestID = b;
    return a >= 0;
  }
  fbr_loop_result performLoopClosure(double timeLaserCloudInfoLast, const fbr_loop_params& lp) {
    fbr_loop_result r{};
    check(fbr_perform_loop_closure(c_.get(), timeLaserCloudInfoLast, &lp, &r), "fbr_perform_loop_closure");
    return r;
  }
  /* pcl::IterativeClosestPoint::align + getFitnessScore on two host clouds. */
  fbr_icp_result icpAlign(const std::vector<fbr_point_xyzi>& source, const std::vector<fbr_point_xyzi>& target,
                          const fbr_icp_params& ip) {
    fbr_icp_result r{};
    check(fbr_icp_align(c_.get(), source.data(), (int64_t)source.size(), target.data(), (int64_t)target.size(), &ip, &r),
          "fbr_icp_align");
    return r;
  }
  /* Loop closure for many keyframe pairs (include/fbr.h, "loop closure for many keyframe pairs"):
   * detectLoopClosure's rule for every keyframe >= firstKeyframe as it stood when that keyframe was
   * the last one; performLoopClosure for an explicit list of pairs, the ICPs of chunkPairs pairs
   * (0: the library's choice) in the same launches, each result the single call's bytes; and
   * icpAlign for many pairs of host clouds. */
  std::vector<fbr_loop_pair> loopCandidates(const fbr_loop_params& lp, int firstKeyframe = 0) {
    int64_t n = 0;
    const int rc = fbr_loop_candidates(c_.get(), &lp, firstKeyframe, nullptr, 0, &n);
    if (rc != FBR_OK && rc != FBR_ERR_CAPACITY) check(rc, "fbr_loop_candidates");
    std::vector<fbr_loop_pair> pairs((size_t)n);
    if (n > 0) check(fbr_loop_candidates(c_.get(), &lp, firstKeyframe, pairs.data(), n, &n), "fbr_loop_candidates");
    return pairs;
  }
  std::vector<fbr_loop_result> performLoopClosures(const std::vector<fbr_loop_pair>& pairs, const fbr_loop_params& lp,
                                                   int chunkPairs = 0) {
    std::vector<fbr_loop_result> r(pairs.size());
    check(fbr_perform_loop_closures(c_.get(), &lp, pairs.data(), (int64_t)pairs.size(), chunkPairs, r.data()),
          "fbr_perform_loop_closures");
    return r;
  }
  std::vector<fbr_icp_result> icpAlignBatch(const std::vector<std::vector<fbr_point_xyzi>>& sources,
                                            const std::vector<std::vector<fbr_point_xyzi>>& targets,
                                            const fbr_icp_params& ip, int chunkPairs = 0) {
    if (sources.size() != targets.size()) throw Error(FBR_ERR_INVALID_ARG, "fbr_icp_align_batch");
    std::vector<const fbr_point_xyzi*> sp, tp;
    std::vector<int64_t> sn, tn;
    for (size_t k = 0; k < sources.size(); ++k) {
      sp.push_back(sources[k].data());
      sn.push_back((int64_t)sources[k].size());
      tp.push_back(targets[k].data());
      tn.push_back((int64_t)targets[k].size());
    }
    std::vector<fbr_icp_result> r(sources.size());
    check(fbr_icp_align_batch(c_.get(), sp.data(), sn.data(), tp.data(), tn.data(), (int64_t)sources.size(), &ip, chunkPairs,
                              r.data()),
          "fbr_icp_align_batch");
    return r;
  }

  /* Place recognition (include/fbr.h, "place recognition"): scan-context descriptors of the
   * keyframes and the exhaustive search over them.  scQuery takes mapping-leaf down-sampled lidar-frame
   * features and returns up to k pose hypotheses in rank order, each to be tried with registration();
   * the *SC loop calls find the revisited place by appearance, so they still work once the drift of
   * the last key pose exceeds historyKeyframeSearchRadius. */
  std::vector<float> scDescribe(const fbr_sc_params& sp, const std::vector<fbr_point_xyzi>& corner,
                                const std::vector<fbr_point_xyzi>& surf) {
    std::vector<float> d((size_t)sp.n_ring * (size_t)sp.n_sector);
    check(fbr_sc_describe(c_.get(), &sp, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size(), d.data()),
          "fbr_sc_describe");
    return d;
  }
  int64_t scUpdate(const fbr_sc_params& sp) {
    int64_t n = 0;
    check(fbr_sc_update(c_.get(), &sp, &n), "fbr_sc_update");
    return n;
  }
  std::vector<float> scDescriptor(const fbr_sc_params& sp, int64_t keyframe) {
    std::vector<float> d((size_t)sp.n_ring * (size_t)sp.n_sector);
    check(fbr_sc_descriptor(c_.get(), keyframe, d.data()), "fbr_sc_descriptor");
    return d;
  }
  std::vector<fbr_sc_match> scQuery(const fbr_sc_params& sp, const std::vector<fbr_point_xyzi>& corner,
                                    const std::vector<fbr_point_xyzi>& surf, int k) {
    std::vector<fbr_sc_match> m((size_t)(k > 0 ? k : 1));
    int n = 0;
    check(fbr_sc_query(c_.get(), &sp, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size(), k, m.data(),
                       &n),
          "fbr_sc_query");
    m.resize((size_t)n);
    return m;
  }
  bool detectLoopClosureSC(double timeLaserCloudInfoLast, const fbr_loop_params& lp, const fbr_sc_params& sp, int* latestID,
                           int* closestID, fbr_sc_match* match = nullptr) {
    int32_t a = -1, b = -1;
    check(fbr_sc_detect_loop_closure(c_.get(), timeLaserCloudInfoLast, &lp, &sp, &a, &b, match),
          "fbr_sc_detect_loop_closure");
    if (latestID) *latestID = a;
    if (closestID) *closestID = b;
    return a >= 0;
  }
  fbr_loop_result performLoopClosureSC(double timeLaserCloudInfoLast, const fbr_loop_params& lp, const fbr_sc_params& sp,
                                       fbr_sc_match* match = nullptr) {
    fbr_loop_result r{};
    check(fbr_perform_loop_closure_sc(c_.get(), timeLaserCloudInfoLast, &lp, &sp, &r, match),
          "fbr_perform_loop_closure_sc");
    return r;
  }

  /* Pose scoring (include/fbr.h, "pose scoring"): how well mapping-leaf down-sampled scan-frame
   * features fit the installed map at each of n poses [roll, pitch, yaw, x, y, z], and the best
   * top_k poses of a lattice of hypotheses around coarse seeds, each to be tried with registration(). */
  std::vector<fbr_pose_score> scorePoses(const fbr_score_params& sp, const std::vector<fbr_point_xyzi>& corner,
                                         const std::vector<fbr_point_xyzi>& surf, const std::vector<float>& poses,
                                         std::vector<uint64_t>* nn_keys = nullptr) {
    const int64_t n = (int64_t)poses.size() / 6;
    std::vector<fbr_pose_score> out((size_t)n);
    if (nn_keys) nn_keys->assign((size_t)n * (corner.size() + surf.size()), ~(uint64_t)0);
    check(fbr_score_poses(c_.get(), &sp, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size(),
                          poses.data(), n, out.data(), nn_keys ? nn_keys->data() : nullptr),
          "fbr_score_poses");
    return out;
  }
  /* Registration information (include/fbr.h, "registration information"): the Gauss-Newton normal
   * matrix of the features at each of n poses, its spectrum and the covariance in the pose graph's
   * chart; batchInfo() the same for every job of the latest batch launch (n_jobs as staged), and
   * infoVariances() the between-factor variances of one record, floored. */
  std::vector<fbr_reg_info> regInfo(const fbr_info_params& ip, const std::vector<fbr_point_xyzi>& corner,
                                    const std::vector<fbr_point_xyzi>& surf, const std::vector<float>& poses) {
    const int64_t n = (int64_t)poses.size() / 6;
    std::vector<fbr_reg_info> out((size_t)n);
    check(fbr_reg_info_poses(c_.get(), &ip, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size(),
                             poses.data(), n, out.data()),
          "fbr_reg_info_poses");
    return out;
  }
  std::vector<fbr_reg_info> batchInfo(const fbr_info_params& ip, int n_jobs) {
    // fbr_batch_info writes one record per job of the launched batch and takes no capacity: room for
    // the context's max_batch, then the caller's n_jobs (the count it staged) are returned
    const int cap = c_.params().max_batch > n_jobs ? c_.params().max_batch : n_jobs;
    std::vector<fbr_reg_info> out((size_t)(cap > 0 ? cap : 1));
    check(fbr_batch_info(c_.get(), &ip, out.data()), "fbr_batch_info");
    out.resize((size_t)(n_jobs > 0 ? n_jobs : 0));
    return out;
  }
  static std::array<double, 6> infoVariances(const fbr_reg_info& info, const double* floor6 = nullptr) {
    std::array<double, 6> v{};
    check(fbr_reg_info_variances(&info, floor6, v.data()), "fbr_reg_info_variances");
    return v;
  }
  struct PoseHypothesis {
    float pose[6];
    fbr_pose_score score;
    int64_t index;  // in the lattice's order
  };
  std::vector<PoseHypothesis> poseSearch(const fbr_score_params& sp, const std::vector<fbr_point_xyzi>& corner,
                                         const std::vector<fbr_point_xyzi>& surf, const std::vector<float>& seeds,
                                         const fbr_pose_lattice& lattice, int64_t top_k) {
    const size_t cap = (size_t)(top_k > 0 ? top_k : 1);
    std::vector<float> poses(cap * 6);
    std::vector<fbr_pose_score> scores(cap);
    std::vector<int64_t> index(cap);
    int64_t n = 0;
    check(fbr_pose_search(c_.get(), &sp, corner.data(), (int64_t)corner.size(), surf.data(), (int64_t)surf.size(),
                          seeds.data(), (int64_t)seeds.size() / 6, &lattice, top_k, poses.data(), scores.data(),
                          index.data(), &n),
          "fbr_pose_search");
    std::vector<PoseHypothesis> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      for (int k = 0; k < 6; ++k) out[(size_t)i].pose[k] = poses[(size_t)i * 6 + k];
      out[(size_t)i].score = scores[(size_t)i];
      out[(size_t)i].index = index[(size_t)i];
    }
    return out;
  }

  /* Pose graph (include/fbr.h, "pose graph"): the factors of saveKeyFramesAndFactor (addOdomFactor
   * :1517-1541, addGPSFactor :1543-1634, the loop BetweenFactor :743-758), a batch optimise in place
   * of isam->update, and correctPoses (:1735-1770) for a host without GTSAM. */
  void pgReset() { check(fbr_pg_reset(c_.get()), "fbr_pg_reset"); }
  void pgAddPrior(int64_t node, const float pose[6], const double variances[6]) {
    check(fbr_pg_add_prior(c_.get(), node, pose, variances), "fbr_pg_add_prior");
  }
  void pgAddBetween(int64_t i, int64_t j, const float between[16], const double variances[6]) {
    check(fbr_pg_add_between(c_.get(), i, j, between, variances), "fbr_pg_add_between");
  }
  void pgAddBetweenPoses(int64_t i, int64_t j, const float pose_i[6], const float pose_j[6], const double variances[6]) {
    check(fbr_pg_add_between_poses(c_.get(), i, j, pose_i, pose_j, variances), "fbr_pg_add_between_poses");
  }
  void pgAddGps(int64_t node, const double xyz[3], const double variances[3]) {
    check(fbr_pg_add_gps(c_.get(), node, xyz, variances), "fbr_pg_add_gps");
  }
  bool pgAddLoop(const fbr_loop_result& r) {
    int added = 0;
    check(fbr_pg_add_loop(c_.get(), &r, &added), "fbr_pg_add_loop");
    return added != 0;
  }
  int64_t pgFactorCount() {
    int64_t n = 0;
    check(fbr_pg_factor_count(c_.get(), &n), "fbr_pg_factor_count");
    return n;
  }
  /* poses (optional) receives [n_nodes][6] doubles = [roll, pitch, yaw, x, y, z]; no key pose changes */
  fbr_pg_result pgOptimize(const fbr_pg_params& pp, std::vector<double>* poses = nullptr) {
    fbr_pg_result r{};
    check(fbr_pg_optimize(c_.get(), &pp, &r), "fbr_pg_optimize");
    if (poses) {
      poses->assign((size_t)r.n_nodes * 6, 0.0);
      int64_t n = 0;
      if (r.n_nodes > 0) check(fbr_pg_poses(c_.get(), poses->data(), r.n_nodes, &n), "fbr_pg_poses");
    }
    return r;
  }
  /* Every loop factor in add order at the last optimise's poses: its index in the factor list, the
   * chi-square |r|^2 of its whitened residual and its robust weight (1 without a robust option). */
  int64_t pgLoopWeights(std::vector<int32_t>* index, std::vector<double>* chi2, std::vector<double>* weight) {
    int64_t n = 0;
    const int rc = fbr_pg_loop_weights(c_.get(), nullptr, nullptr, nullptr, 0, &n);
    if (rc != FBR_OK && rc != FBR_ERR_CAPACITY) check(rc, "fbr_pg_loop_weights");
    index->assign((size_t)n, 0);
    chi2->assign((size_t)n, 0.0);
    weight->assign((size_t)n, 0.0);
    if (n > 0) check(fbr_pg_loop_weights(c_.get(), index->data(), chi2->data(), weight->data(), n, &n), "fbr_pg_loop_weights");
    return n;
  }
  void correctPoses() { check(fbr_pg_apply(c_.get()), "fbr_pg_apply"); }
  /* poseCovariance (:1706) of the key poses `nodes` (empty: every node, n of them) at the last
   * optimise's poses: cov [rows][36] row-major, tangent order [rotation; translation]. */
  fbr_pg_marginal_result pgMarginals(std::vector<double>* cov, const std::vector<int64_t>& nodes = {}, int64_t n = 0,
                                     const fbr_pg_marginal_params* mp = nullptr) {
    fbr_pg_marginal_params p;
    fbr_pg_marginal_params_default(&p);
    if (mp) p = *mp;
    fbr_pg_marginal_result r{};
    const int64_t rows = nodes.empty() ? n : (int64_t)nodes.size();
    cov->assign((size_t)rows * 36, 0.0);
    check(fbr_pg_marginals(c_.get(), &p, nodes.empty() ? nullptr : nodes.data(), rows, cov->data(), rows, &r),
          "fbr_pg_marginals");
    return r;
  }
  /* addGPSFactor's covariance gate (:1561) on the last key pose. */
  bool pgGpsGate(double poseCovThreshold, double cov_xy[2] = nullptr) {
    int wanted = 0;
    check(fbr_pg_gps_gate(c_.get(), poseCovThreshold, &wanted, cov_xy), "fbr_pg_gps_gate");
    return wanted != 0;
  }

  /* visualizeGlobalMapThread's save block (:485-521) in three steps: build the global map from the
   * keyframe store (params null: the reference's mode; wide = 1 is this project's extension for maps
   * PCL's VoxelGrid refuses), read it back or install it as the registration map without leaving
   * the device, and write the reference's files into an existing directory. */
  fbr_gmap_result buildGlobalMap(const fbr_gmap_params* params = nullptr) {
    fbr_gmap_result r{};
    check(fbr_global_map_build(c_.get(), params, &r), "fbr_global_map_build");
    return r;
  }
  void globalMap(std::vector<fbr_point_xyzi>* corner, std::vector<fbr_point_xyzi>* surf) {
    int64_t nc = 0, ns = 0;
    check(fbr_global_map_get(c_.get(), &nc, &ns, nullptr, nullptr), "fbr_global_map_get");
    if (corner) corner->assign((size_t)nc, fbr_point_xyzi{});
    if (surf) surf->assign((size_t)ns, fbr_point_xyzi{});
    check(fbr_global_map_get(c_.get(), nullptr, nullptr, corner && nc ? corner->data() : nullptr,
                             surf && ns ? surf->data() : nullptr),
          "fbr_global_map_get");
  }
  void installGlobalMap() { check(fbr_global_map_install(c_.get()), "fbr_global_map_install"); }
  void saveGlobalMap(const std::string& dir, bool cloud_global = false) {
    check(fbr_global_map_save(c_.get(), dir.c_str(), cloud_global ? FBR_GMAP_SAVE_GLOBAL : 0), "fbr_global_map_save");
  }

 private:
  Context& c_;
  double timeLastProcessing_ = -1.0;  // mapOptmization.h:135 (timeLastProcessing = -1)
  fbr_reg_stats stats_{};
};

/* The node-level chain of cloudHandler (:182-226): project -> featureExtra -> registration with
 * the static pose (step = identity, so pose = pose * step = pose). */
class Node {
 public:
  explicit Node(Context& c) : proj_(c), feat_(c), map_(c), pose_(Affine3f::Identity()) {}
  MapOptimization& matcher() { return map_; }
  const Affine3f& pose() const { return pose_; }
  void setPose(const Affine3f& p) { pose_ = p; }
  const CloudInfo& cloudInfo() const { return info_; }

  bool cloudHandler(const fbr_point_xyzirt* pts, int64_t n, double stamp) {
    if (!proj_.cloudHandler(pts, n, stamp, info_)) return false;
    feat_.featureExtra(info_);
    map_.registration(info_, pose_);
    return true;
  }
  /* The reference's entry point proper: cloudHandler(const sensor_msgs::PointCloud2ConstPtr&)
   * (:182-226), including the 2-message cache queue (returns false while it fills). */
  bool cloudHandler(const PointCloud2& msg) {
    if (!proj_.cloudHandler(msg, info_)) return false;
    feat_.featureExtra(info_);
    map_.registration(info_, pose_);
    return true;
  }
  ImageProjection& projection() { return proj_; }

 private:
  ImageProjection proj_;
  FeatureExtraction feat_;
  MapOptimization map_;
  Affine3f pose_;
  CloudInfo info_;
};

}  // namespace fbr

#endif /* FBR_HPP_ */
