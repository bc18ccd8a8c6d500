// fbr_motion.h — motion deskew arithmetic (fbr_set_motion), shared by the host entry points
// (fbr_odom.cpp), the device kernels (k_project.hip) and the tests' host probe.  It sits beside
// fbr_imu.h and restates deskewPoint (the reference's src/imageProjection.cpp:545-580) with
// findPosition's commented body (:528-542) live:
//   ratio (time from the field)   (float)(relTime / (timeScanNext - timeScanCur)), relTime =
//                                 (double)point.time; the division in double (:537)
//   ratio (time from the column)  (float)k / (float)W, k = (direction * (col - col_first)) mod W in
//                                 [0, W): a spinning sensor sweeps its columns at a constant rate
//   pos                           ratio * odomIncre{X, Y, Z}, a float product per axis (:539-541)
//   rot                           findRotation's (fbr_imu.h) with an IMU table; else, with
//                                 FBR_MOTION_ROTATION, ratio * {roll, pitch, yaw}Incre: the linear
//                                 interpolation of Euler angles findRotation applies to the gyro's
//   transFinal                    pcl::getTransformation(pos, rot)
//   transStartInverse             transFinal(first point).inverse(): Eigen's Affine inverse with a
//                                 translation, t' = (-L^-1) * t
//   transBt                       transStartInverse * transFinal: L = L1 * L2, t = L1 * t2 + t1
// 3-term sums are x0 + (x1 + x2) as in fbr_imu.h; no FMA contraction.
// At t = +0 the general inverse and product below evaluate the expressions of fbr_imu.h's
// affine_inverse / compose term by term ((-inv) * 0, l1 * 0), so they give the same bits; the IMU
// path keeps calling the zero-translation pair all the same.
#pragma once
#include "fbr_imu.h"

namespace fbr {

// desk_mode bits of a job (fbr_set_motion), beside kDeskPoints / kDeskImu
constexpr int kDeskMotPos = 4;   // FBR_MOTION_POSITION
constexpr int kDeskMotRot = 8;   // FBR_MOTION_ROTATION
constexpr int kDeskMotCol = 16;  // FBR_TIME_COLUMN
constexpr int kDeskMotion = kDeskMotPos | kDeskMotRot;

FBR_HD inline int motion_mode_bits(const fbr_motion& m) {
  if (!m.flags) return 0;
  return ((m.flags & FBR_MOTION_POSITION) ? kDeskMotPos : 0) | ((m.flags & FBR_MOTION_ROTATION) ? kDeskMotRot : 0) |
         (m.time_source == FBR_TIME_COLUMN ? kDeskMotCol : 0);
}

FBR_HD inline float motion_ratio_field(float time, double scan_period) { return (float)((double)time / scan_period); }

// k of a column: how many columns after the scan's first kept point the sensor fires it
FBR_HD inline int motion_column_k(int direction, int col, int col_first, int W) {
  int k = (direction * (col - col_first)) % W;
  return k < 0 ? k + W : k;
}
FBR_HD inline float motion_ratio_column(int k, int W) { return (float)k / (float)W; }

// A 3x4 affine transform: linear part and translation.
struct Aff3 {
  Rot3 r;
  float t[3];
};

// Affine3f::inverse() with a translation: the cofactor inverse of fbr_imu.h, t' = (-L^-1) * t.
FBR_HD inline void affine_inverse_t(const Rot3& a, const float t[3], Rot3& inv, float tout[3]) {
  float z[3];
  affine_inverse(a, inv, z);
  for (int r = 0; r < 3; ++r) tout[r] = sum3(-inv.m[r][0] * t[0], -inv.m[r][1] * t[1], -inv.m[r][2] * t[2]);
}

// Affine3f * Affine3f: L = L1 * L2, t = L1 * t2 + t1.
FBR_HD inline void compose_t(const Rot3& l1, const float t1[3], const Rot3& r, const float t2[3], Rot3& out,
                             float tout[3]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out.m[i][j] = sum3(l1.m[i][0] * r.m[0][j], l1.m[i][1] * r.m[1][j], l1.m[i][2] * r.m[2][j]);
    tout[i] = sum3(l1.m[i][0] * t2[0], l1.m[i][1] * t2[1], l1.m[i][2] * t2[2]) + t1[i];
  }
}

// findPosition live and the rotation choice.  rot holds findRotation's angles when imu is set (left
// as they are); bits are the job's kDeskMot* bits.
FBR_HD inline void motion_pos_rot(const float incre[6], int bits, float ratio, bool imu, float rot[3], float pos[3]) {
  for (int a = 0; a < 3; ++a) {
    pos[a] = (bits & kDeskMotPos) ? ratio * incre[3 + a] : 0.0f;
    if (!imu) rot[a] = (bits & kDeskMotRot) ? ratio * incre[a] : 0.0f;
  }
}

// transFinal = pcl::getTransformation(pos, rot)
FBR_HD inline Aff3 motion_trans_final(const float rot[3], const float pos[3]) {
  Aff3 f;
  f.r = rot_rpy(rot[0], rot[1], rot[2]);
  f.t[0] = pos[0];
  f.t[1] = pos[1];
  f.t[2] = pos[2];
  return f;
}

// transStartInverse from the first point's transFinal.
FBR_HD inline Aff3 motion_start_inverse(const Aff3& first) {
  Aff3 s;
  affine_inverse_t(first.r, first.t, s.r, s.t);
  return s;
}

// transBt = transStartInverse * transFinal
FBR_HD inline Aff3 motion_trans_bt(const Aff3& start_inv, const Aff3& fin) {
  Aff3 b;
  compose_t(start_inv.r, start_inv.t, fin.r, fin.t, b.r, b.t);
  return b;
}

// The whole of deskewPoint for a job without an IMU table: the transform of a point at `ratio`
// in a scan whose first point is at `ratio_first`.
FBR_HD inline Aff3 motion_transform(const float incre[6], int bits, float ratio_first, float ratio) {
  float rot[3], pos[3];
  motion_pos_rot(incre, bits, ratio_first, false, rot, pos);
  const Aff3 s = motion_start_inverse(motion_trans_final(rot, pos));
  motion_pos_rot(incre, bits, ratio, false, rot, pos);
  return motion_trans_bt(s, motion_trans_final(rot, pos));
}

// ---- pose algebra of the host entry points (float, as pcl / Eigen compute it) ----
// pcl::getTransformation(x, y, z, roll, pitch, yaw) of a pose {roll, pitch, yaw, x, y, z}
FBR_HD inline Aff3 aff_from_pose(const float p[6]) {
  const float rot[3] = {p[0], p[1], p[2]}, pos[3] = {p[3], p[4], p[5]};
  return motion_trans_final(rot, pos);
}

}  // namespace fbr
