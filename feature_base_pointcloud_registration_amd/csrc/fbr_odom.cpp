// fbr_odom.cpp — host side of the motion path (fbr_motion.h): odomDeskewInfo
// (src/imageProjection.cpp:395-491 of the reference), the constant-velocity motion record from two
// registered poses, and updateInitialGuess (src/mapOptmization.h:799-855).  No device is needed.
// Third-party semantics restated:
//   tf::quaternionMsgToTF              normalises when |length2 - 1| > QUATERNION_TOLERANCE (0.1)
//   tf::Matrix3x3(q).getRPY            fbr_imu.h (double)
//   pcl::getTransformation             fbr_imu.h rot_rpy (float; glibc sinf / cosf)
//   pcl::getTranslationAndEulerAngles  roll = atan2f(m21, m22), pitch = asinf(-m20),
//                                      yaw = atan2f(m10, m00) (float)
//   Affine3f::inverse, Affine3f * Affine3f   fbr_motion.h
#include <cmath>
#include <cstring>

#include "fbr.h"
#include "fbr_motion.h"

namespace {

using fbr::Aff3;

void odom_rpy(const fbr_odom_sample& s, double* roll, double* pitch, double* yaw) {
  fbr::TfQuat q{s.orientation[0], s.orientation[1], s.orientation[2], s.orientation[3]};
  const double l2 = fbr::tf_dot(q, q);
  if (std::fabs(l2 - 1) > 0.1f) {  // QUATERNION_TOLERANCE: normalize() = *this *= 1 / length()
    const double inv = 1.0 / std::sqrt(l2);
    q.x *= inv;
    q.y *= inv;
    q.z *= inv;
    q.w *= inv;
  }
  fbr::tf_get_rpy(q, roll, pitch, yaw);
}

// pcl::getTranslationAndEulerAngles into {roll, pitch, yaw, x, y, z}
void pose_from_aff(const Aff3& a, float p[6]) {
  p[3] = a.t[0];
  p[4] = a.t[1];
  p[5] = a.t[2];
  p[0] = std::atan2(a.r.m[2][1], a.r.m[2][2]);
  p[1] = std::asin(-a.r.m[2][0]);
  p[2] = std::atan2(a.r.m[1][0], a.r.m[0][0]);
}

// pcl::getTransformation of a sample's position (double -> float arguments) and its roll, pitch, yaw
Aff3 aff_from_sample(const fbr_odom_sample& s, double roll, double pitch, double yaw) {
  const float p[6] = {(float)roll, (float)pitch, (float)yaw, (float)s.position[0], (float)s.position[1],
                      (float)s.position[2]};
  return fbr::aff_from_pose(p);
}

Aff3 aff_inverse(const Aff3& a) { return fbr::motion_start_inverse(a); }
Aff3 aff_mul(const Aff3& a, const Aff3& b) { return fbr::motion_trans_bt(a, b); }

bool finite6(const float* p) {
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}

void motion_clear(fbr_motion* m, double scan_period) {
  std::memset(m, 0, sizeof(*m));
  m->time_source = FBR_TIME_FIELD;
  m->column_direction = 1;
  m->scan_period = scan_period;
}

}  // namespace

extern "C" {

int fbr_odom_deskew_info(const fbr_odom_sample* q, int64_t n, double timeScanCur, double timeScanNext,
                         fbr_odom_info* out, int64_t* n_pop) {
  if (!out || n < 0 || (n && !q)) return FBR_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  motion_clear(&out->motion, timeScanNext - timeScanCur);
  if (n_pop) *n_pop = 0;
  // cloudInfo.odomAvailable = false; pop_front while stamp < timeScanCur - 0.01 (:397-405)
  int64_t b = 0;
  while (b < n && q[b].stamp < timeScanCur - 0.01) ++b;
  if (n_pop) *n_pop = b;
  if (b == n) return FBR_OK;                      // :407-408
  if (q[b].stamp > timeScanCur) return FBR_OK;    // :410-411
  // the start sample: the first with stamp >= timeScanCur, the last one when none qualifies (:418-428)
  int64_t is = b;
  for (int64_t i = b; i < n; ++i) {
    is = i;
    if (q[i].stamp < timeScanCur) continue;
    break;
  }
  const fbr_odom_sample& s0 = q[is];
  double roll, pitch, yaw;
  odom_rpy(s0, &roll, &pitch, &yaw);
  out->initial_guess[0] = (float)roll;  // :439-445
  out->initial_guess[1] = (float)pitch;
  out->initial_guess[2] = (float)yaw;
  out->initial_guess[3] = (float)s0.position[0];
  out->initial_guess[4] = (float)s0.position[1];
  out->initial_guess[5] = (float)s0.position[2];
  out->reset_id = (int32_t)std::round(s0.covariance0);
  out->odom_available = 1;
  // the end sample (:451-472)
  if (q[n - 1].stamp < timeScanNext) return FBR_OK;
  int64_t ie = b;
  for (int64_t i = b; i < n; ++i) {
    ie = i;
    if (q[i].stamp < timeScanNext) continue;
    break;
  }
  const fbr_odom_sample& s1 = q[ie];
  if ((int)std::round(s0.covariance0) != (int)std::round(s1.covariance0)) return FBR_OK;
  const Aff3 transBegin = aff_from_sample(s0, roll, pitch, yaw);
  odom_rpy(s1, &roll, &pitch, &yaw);
  const Aff3 transEnd = aff_from_sample(s1, roll, pitch, yaw);
  const Aff3 transBt = aff_mul(aff_inverse(transBegin), transEnd);  // :484
  pose_from_aff(transBt, out->motion.incre);                         // :488
  out->odom_deskew_flag = 1;
  return FBR_OK;
}

int fbr_motion_from_poses(const float prev[6], const float cur[6], double dt, double scan_period, double dt_next,
                          fbr_motion* out, float guess_out[6]) {
  if (!prev || !cur || !finite6(prev) || !finite6(cur)) return FBR_ERR_INVALID_ARG;
  if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite(scan_period) || !std::isfinite(dt_next))
    return FBR_ERR_INVALID_ARG;
  if (out && !(scan_period > 0.0)) return FBR_ERR_INVALID_ARG;
  const Aff3 a = fbr::aff_from_pose(prev), b = fbr::aff_from_pose(cur);
  float step[6];
  pose_from_aff(aff_mul(aff_inverse(a), b), step);
  if (out) {
    motion_clear(out, scan_period);
    out->flags = FBR_MOTION_POSITION | FBR_MOTION_ROTATION;
    for (int k = 0; k < 6; ++k) out->incre[k] = (float)((double)step[k] * (scan_period / dt));
  }
  if (guess_out) {
    float nxt[6];
    for (int k = 0; k < 6; ++k) nxt[k] = (float)((double)step[k] * (dt_next / dt));
    pose_from_aff(aff_mul(b, fbr::aff_from_pose(nxt)), guess_out);
  }
  return FBR_OK;
}

int fbr_update_initial_guess(fbr_guess_state* st, const fbr_odom_info* odom, const fbr_deskew_table* table,
                             int have_keyframes, int use_imu_heading, float tr[6]) {
  if (!st || !tr) return FBR_ERR_INVALID_ARG;
  const float ri = table ? table->imu_roll_init : 0.0f, pi = table ? table->imu_pitch_init : 0.0f,
              yi = table ? table->imu_yaw_init : 0.0f;
  auto save_imu = [&]() {  // lastImuTransformation = getTransformation(0, 0, 0, imu*Init)
    const float p[6] = {ri, pi, yi, 0.0f, 0.0f, 0.0f};
    const Aff3 a = fbr::aff_from_pose(p);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) st->last_imu[4 * r + c] = a.r.m[r][c];
      st->last_imu[4 * r + 3] = a.t[r];
    }
  };
  if (!have_keyframes) {  // :804-818
    tr[0] = ri;
    tr[1] = pi;
    tr[2] = yi;
    if (!use_imu_heading) tr[2] = 0;
    save_imu();
    return FBR_OK;
  }
  if (odom && odom->odom_available && odom->reset_id == st->reset_id) {  // :823-835
    for (int k = 0; k < 6; ++k) tr[k] = odom->initial_guess[k];
    save_imu();
    return FBR_OK;
  }
  if (table && table->imu_available) {  // :839-854
    const float p[6] = {ri, pi, yi, 0.0f, 0.0f, 0.0f};
    const Aff3 transBack = fbr::aff_from_pose(p);
    Aff3 last;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) last.r.m[r][c] = st->last_imu[4 * r + c];
      last.t[r] = st->last_imu[4 * r + 3];
    }
    const Aff3 transIncre = aff_mul(aff_inverse(last), transBack);
    const Aff3 transFinal = aff_mul(fbr::aff_from_pose(tr), transIncre);
    pose_from_aff(transFinal, tr);
    save_imu();
  }
  return FBR_OK;
}

}  // extern "C"
