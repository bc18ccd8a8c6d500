// motion_probe.cpp — csrc/fbr_motion.h compiled for the host (tests/test_motion_model.py,
// tests/test_motion_deskew.py): the ratios, and deskewPoint with findPosition live, point by point.
#include <cstdint>

#include "fbr.h"
#include "fbr_motion.h"

using namespace fbr;

extern "C" {

void mp_ratio_field(const float* time, double scan_period, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = motion_ratio_field(time[i], scan_period);
}

void mp_ratio_column(const int32_t* col, int col_first, int direction, int W, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = motion_ratio_column(motion_column_k(direction, col[i], col_first, W), W);
}

// flags: FBR_MOTION_* of the record.  incre [n][6] when per_case, else [6]; ratio_first [n] when
// per_case, else [1].  xyz, out: [n][3].
void mp_deskew(const float* incre, int flags, int per_case, const float* ratio_first, const float* ratio,
               const float* xyz, float* out, int64_t n) {
  fbr_motion m{};
  m.flags = flags;
  const int bits = motion_mode_bits(m);
  for (int64_t i = 0; i < n; ++i) {
    const float* inc = per_case ? incre + 6 * i : incre;
    const Aff3 T = motion_transform(inc, bits, per_case ? ratio_first[i] : ratio_first[0], ratio[i]);
    apply_affine(T.r, T.t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out + 3 * i);
  }
}

// The same on a job with an IMU table: the rotation is findRotation's at time_scan_cur + time, the
// translation the motion's.
void mp_deskew_imu(const fbr_deskew_table* T, const float* incre, int flags, float time_first, float ratio_first,
                   const float* time, const float* ratio, const float* xyz, float* out, int64_t n) {
  fbr_motion m{};
  m.flags = flags;
  const int bits = motion_mode_bits(m);
  float rot[3], pos[3];
  find_rotation(*T, T->time_scan_cur + (double)time_first, &rot[0], &rot[1], &rot[2]);
  motion_pos_rot(incre, bits, ratio_first, true, rot, pos);
  const Aff3 s = motion_start_inverse(motion_trans_final(rot, pos));
  for (int64_t i = 0; i < n; ++i) {
    find_rotation(*T, T->time_scan_cur + (double)time[i], &rot[0], &rot[1], &rot[2]);
    motion_pos_rot(incre, bits, ratio[i], true, rot, pos);
    const Aff3 b = motion_trans_bt(s, motion_trans_final(rot, pos));
    apply_affine(b.r, b.t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out + 3 * i);
  }
}

// fbr_imu.h's zero-translation pair against the general one at t = +0 (bit comparison in the test)
void mp_zero_t_pair(float roll, float pitch, float yaw, float* old12, float* new12) {
  const Rot3 R = rot_rpy(roll, pitch, yaw);
  const float z[3] = {0.0f, 0.0f, 0.0f};
  Rot3 a, b, ca, cb;
  float ta[3], tb[3], ua[3], ub[3];
  affine_inverse(R, a, ta);
  affine_inverse_t(R, z, b, tb);
  compose(a, ta, R, ca, ua);
  compose_t(b, tb, R, z, cb, ub);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      old12[4 * i + j] = ca.m[i][j];
      new12[4 * i + j] = cb.m[i][j];
    }
    old12[4 * i + 3] = ua[i];
    new12[4 * i + 3] = ub[i];
  }
}

}  // extern "C"
