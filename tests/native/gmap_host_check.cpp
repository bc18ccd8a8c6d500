// Stand-alone host check (its own main; built with -fsanitize=address,undefined by
// tests/test_gmap_model.py, never loaded into Python, never run on a GPU): csrc/fbr_gmap.h's grid
// and key code over ordinary, overflowing, refused and degenerate boxes, and
// fbr_pcd_write_poses_ascii (csrc/fbr_pcd.cpp, compiled into this program) writing and re-reading
// a file.  Prints "gmap_host_check: ok" and exits 0 when every check holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "fbr.h"
#include "fbr_gmap.h"

// fbr_pcd.cpp's fbr_load_map refers to it; nothing here calls either
extern "C" int fbr_set_map(fbr_ctx*, const fbr_point_xyzi*, int64_t, const fbr_point_xyzi*, int64_t) { return FBR_ERR_NO_DEVICE; }

static int fails = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static uint32_t rng_state = 12345u;
static float frand(float lo, float hi) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * (float)(rng_state >> 8) / 16777216.0f;
}

// A cloud inside [mn, mx] with both corners present: every key below 2^nbits, equal cells equal keys.
static void check_box(const float mn[3], const float mx[3], float leaf, int32_t want_status, int32_t want_overflow) {
  fbr::GmapGrid G;
  fbr::gmap_grid_init(G, mn, mx, leaf);
  CHECK(G.status == want_status);
  CHECK(G.pcl_overflow == want_overflow);
  if (G.status != fbr::kGmapOk) return;
  CHECK(G.nbits >= 1 && G.nbits <= 63);
  const uint64_t drop = fbr::gmap_drop_key(G);
  CHECK(fbr::gmap_key(G, mn[0], mn[1], mn[2]) == 0);
  const uint64_t kmax = fbr::gmap_key(G, mx[0], mx[1], mx[2]);
  CHECK(kmax < drop);
  CHECK(kmax == (uint64_t)(G.div_b[0] - 1) + (uint64_t)(G.div_b[1] - 1) * G.mul1 + (uint64_t)(G.div_b[2] - 1) * G.mul2);
  for (int i = 0; i < 2000; ++i) {
    const float x = frand(mn[0], mx[0]), y = frand(mn[1], mx[1]), z = frand(mn[2], mx[2]);
    if (x < mn[0] || x > mx[0] || y < mn[1] || y > mx[1] || z < mn[2] || z > mx[2]) continue;
    const uint64_t k = fbr::gmap_key(G, x, y, z);
    CHECK(k <= kmax);
    const uint64_t k2 = k / G.mul2, r = k - k2 * G.mul2, k1 = r / G.mul1, k0 = r - k1 * G.mul1;
    CHECK(k0 < (uint64_t)G.div_b[0] && k1 < (uint64_t)G.div_b[1] && k2 < (uint64_t)G.div_b[2]);
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  {
    const float a[3] = {-12.5f, -9.25f, -2.0f}, b[3] = {12.0f, 9.0f, 3.5f};
    check_box(a, b, 0.2f, fbr::kGmapOk, 0);
    check_box(a, b, 0.4f, fbr::kGmapOk, 0);
    check_box(a, a, 0.2f, fbr::kGmapOk, 0);  // one cell
  }
  {
    const float a[3] = {-1.0f, -1.0f, -1.0f}, b[3] = {301.0f, 301.0f, 241.0f}, c[3] = {2001.0f, 2001.0f, 201.0f};
    check_box(a, b, 0.2f, fbr::kGmapOk, 1);  // 2^31 .. 2^32 cells
    check_box(a, c, 0.2f, fbr::kGmapOk, 1);  // above 2^32 cells
  }
  {
    const float a[3] = {-3.0e5f, -3.0e5f, -3.0e5f}, b[3] = {3.0e5f, 3.0e5f, 3.0e5f};
    check_box(a, b, 0.2f, fbr::kGmapCells, 1);  // 2^64.5 cells
    const float z[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.2f * 2097151.0f, 0.2f * 2097151.0f, 0.2f * 1048575.0f};
    check_box(z, c, 0.2f, fbr::kGmapOk, 1);  // 2^62 cells: the widest key
  }
  {
    const float far = 0.2f * 16777216.0f + 100.0f;
    const float a[3] = {far, 0.0f, 0.0f}, b[3] = {far + 5.0f, 5.0f, 5.0f};
    check_box(a, b, 0.2f, fbr::kGmapBound, 0);
    const float c[3] = {0.0f, 0.0f, -inf}, d[3] = {1.0f, 1.0f, inf}, e[3] = {0.0f, nan, 0.0f};
    check_box(c, d, 0.2f, fbr::kGmapBound, 1);
    check_box(e, b, 0.2f, fbr::kGmapBound, 1);
    const float f[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, g[3] = {3.0e38f, 3.0e38f, 3.0e38f};
    check_box(f, g, 1.0e-3f, fbr::kGmapBound, 1);  // every product overflows to infinity
  }
  CHECK(!fbr::gmap_finite(nan) && !fbr::gmap_finite(inf) && !fbr::gmap_finite(-inf) && fbr::gmap_finite(3.4e38f));
  {
    const float T[12] = {0.0f, -1.0f, 0.0f, 10.0f, 1.0f, 0.0f, 0.0f, -20.0f, 0.0f, 0.0f, 1.0f, 0.5f};
    float x, y, z;
    fbr::gmap_transform(T, 1.0f, 2.0f, 3.0f, &x, &y, &z);
    CHECK(x == 8.0f && y == -19.0f && z == 3.5f);
  }
  // the pose writer: 0, 1 and 3 poses, a NaN, a time above 1e9; read back through fbr_pcd_read
  {
    const char* tmp = getenv("TMPDIR");
    const std::string path = std::string(tmp ? tmp : "/tmp") + "/gmap_host_check_poses.pcd";
    std::vector<fbr_keypose> poses(3);
    memset(poses.data(), 0, sizeof(fbr_keypose) * poses.size());
    poses[0].x = 1.5f;
    poses[1].y = nan;
    poses[1].time = 1700000000.123456;
    poses[2].z = -7.25f;
    poses[2].intensity = 2.0f;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)3}) {
      CHECK(fbr_pcd_write_poses_ascii(path.c_str(), n ? poses.data() : nullptr, n) == FBR_OK);
      int64_t m = -1;
      CHECK(fbr_pcd_read(path.c_str(), nullptr, 0, &m) == FBR_OK && m == n);
      std::vector<fbr_point_xyzi> back((size_t)n + 1);
      CHECK(fbr_pcd_read(path.c_str(), back.data(), n, &m) == FBR_OK && m == n);
      if (n == 3) CHECK(back[0].x == 1.5f && isnan(back[1].y) && back[2].z == -7.25f && back[2].intensity == 2.0f);
    }
    CHECK(fbr_pcd_write_poses_ascii(nullptr, poses.data(), 1) == FBR_ERR_INVALID_ARG);
    CHECK(fbr_pcd_write_poses_ascii(path.c_str(), nullptr, 1) == FBR_ERR_INVALID_ARG);
    CHECK(fbr_pcd_write_poses_ascii((path + "/no/such").c_str(), poses.data(), 1) == FBR_ERR_INVALID_ARG);
    remove(path.c_str());
  }
  if (fails) return 1;
  printf("gmap_host_check: ok\n");
  return 0;
}
