// Host check of the temporal-stereo arithmetic (csrc/temporal_math.h, the text the kernels of csrc/temporal.hip compile): the
// projection under the identity and under a forward move, the keep test on NaN, infinities, points behind the camera and
// targets outside the image (nothing is converted to int before it is compared), the key's order and its round trip with
// the tie rule, the visibility test, the payload, and the five cases of the fusion with the gate at equality.  Plain C++, no
// device, no HIP header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <package>/csrc \
//       tools/temporal_math_check.cpp -o temporal_check && ./temporal_check
// Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "temporal_math.h"

namespace {

int failures = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++failures;                                         \
    }                                                     \
  } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNan = std::numeric_limits<float>::quiet_NaN();

TmProj identity(int H, int W) {
  TmProj p = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 0.f, 0.0625f, 64.f, 0.125f, H, W};
  return p;
}

void check_identity() {
  const TmProj p = identity(37, 53);
  std::vector<unsigned long long> ws((size_t)p.H * p.W, 0ull);   // every target is written through a checked index
  for (int v = 0; v < p.H; ++v)
    for (int u = 0; u < p.W; ++u) {
      const float d = 0.5f + 0.37f * (float)u + 0.011f * (float)v;
      long target = -1;
      float denp = -1.f;
      const bool keep = tm_project(p, u, v, d, &target, &denp);
      CHECK(keep == (d < p.max_disp), "u %d v %d", u, v);
      if (!keep) continue;
      CHECK(target == (long)v * p.W + u && tm_bits(denp) == tm_bits(d), "u %d v %d target %ld", u, v, target);
      CHECK(tm_ratio(p, u, v, d) == 1.f, "ratio");
      ws.at((size_t)target) = tm_key(denp, target);
      CHECK(tm_key_src(ws.at((size_t)target)) == target && tm_bits(tm_key_den(ws.at((size_t)target))) == tm_bits(d), "round trip");
    }
}

void check_refused_pixels() {
  TmProj p = identity(20, 30);
  long target = -1;
  float denp = -1.f;
  for (float d : {kNan, kInf, -kInf, 0.f, -0.f, -3.f, 0.06f, 64.f, 1e30f})
    CHECK(!tm_project(p, 3, 4, d, &target, &denp), "d %g", (double)d);
  CHECK(target == -1 && denp == -1.f, "a refused pixel writes nothing");
  CHECK(tm_project(p, 3, 4, 0.0625f, &target, &denp) && target == 4 * 30 + 3, "the smallest valid disparity");
  // the target leaves the image on every side, and by far (1e30 pixels: no int sees it)
  for (float shift : {-5.f, 27.f, -1e30f, 1e30f, kInf}) {
    p = identity(20, 30);
    p.g[2] = shift;
    CHECK(!tm_project(p, 3, 4, 5.f, &target, &denp), "column shift %g", (double)shift);
    p = identity(20, 30);
    p.g[6] = shift;
    CHECK(!tm_project(p, 3, 4, 5.f, &target, &denp), "row shift %g", (double)shift);
  }
  p = identity(20, 30);
  p.g[2] = -3.4f;                                                   // 3 - 3.4 = -0.4 rounds to column 0: still inside
  CHECK(tm_project(p, 3, 4, 5.f, &target, &denp) && target == 4 * 30, "rounding to the first column");
  p.g[2] = -3.6f;
  CHECK(!tm_project(p, 3, 4, 5.f, &target, &denp), "rounding past the first column");
  // the depth ratio: too close, on the camera plane, behind it
  for (float z : {0.1f, 0.f, -0.f, -1.f, kNan}) {
    p = identity(20, 30);
    p.g[10] = z;
    CHECK(!tm_project(p, 3, 4, 5.f, &target, &denp), "ratio %g", (double)z);
    p.min_ratio = 0.f;
    if (!(z > 0.f)) CHECK(!tm_project(p, 3, 4, 5.f, &target, &denp), "ratio %g without a limit", (double)z);
  }
  // forward by a tenth of the depth: the pixel moves away from the centre, the disparity grows by 1 / 0.9
  p = identity(20, 30);
  p.g[11] = -0.1f / 5.f;                                            // z = 1 - 0.02 den
  CHECK(tm_project(p, 20, 10, 5.f, &target, &denp), "forward");
  CHECK(target == 11 * 30 + 22 && std::fabs(denp - 5.f / 0.9f) < 1e-5f, "forward: target %ld den' %g", target, (double)denp);
}

void check_key_order() {
  const float dens[] = {0.f, 1e-30f, 0.0625f, 1.f, 1.0000001f, 63.999f, 1e30f};
  for (size_t i = 0; i + 1 < sizeof dens / sizeof *dens; ++i) {
    CHECK(tm_key(dens[i], 0) < tm_key(dens[i + 1], 2147483646L), "the nearer surface wins whatever the index: %zu", i);
    CHECK(tm_key(dens[i], 5) > tm_key(dens[i], 6), "among equal den' the smaller source index wins: %zu", i);
  }
  CHECK(tm_key(0.f, 2147483646L) != 0ull, "a kept pixel's key is never the cleared word");
  CHECK(tm_key_src(tm_key(3.5f, 2147483646L)) == 2147483646L, "the largest index");
  CHECK(tm_visible(3.f, 1.f, 4.f) && !tm_visible(3.f, 1.f, 4.0000005f) && tm_visible(3.f, 0.f, 3.f), "the threshold is inclusive");
  CHECK(tm_visible(3.f, 1.f, 0.f), "an empty neighbourhood hides nothing");
}

void check_payload() {
  CHECK(tm_pred_age(0) == 1 && tm_pred_age(254) == 255 && tm_pred_age(255) == 255, "the age saturates");
  CHECK(tm_pred_var(0.25f, 1.f, 0.f) == 0.25f && tm_pred_var(0.25f, 0.5f, 0.125f) == 1.125f, "var / z^2 + q");
}

void check_fuse() {
  TmState r = tm_fuse(false, 5.f, 0.25f, false, 4.f, 0.5f, 7, 9.f);
  CHECK(r.disp == 0.f && r.var == 0.f && r.age == 0 && r.innov == 0.f, "neither");
  r = tm_fuse(true, 5.f, 0.25f, false, 4.f, 0.5f, 7, 9.f);
  CHECK(r.disp == 5.f && r.var == 0.25f && r.age == 0 && r.innov == 0.f, "only the measurement");
  r = tm_fuse(false, 5.f, 0.25f, true, 4.f, 0.5f, 7, 9.f);
  CHECK(r.disp == 4.f && r.var == 0.5f && r.age == 7 && r.innov == 0.f, "coast");
  r = tm_fuse(true, 5.f, 0.25f, true, 4.f, 0.25f, 7, 9.f);
  CHECK(r.disp == 4.5f && r.var == 0.125f && r.age == 7 && r.innov == 1.f, "two equal variances: the mean, half the variance");
  r = tm_fuse(true, 7.f, 0.25f, true, 4.f, 0.25f, 7, 9.f);
  CHECK(r.disp == 7.f && r.var == 0.25f && r.age == 0 && r.innov == 3.f, "9 > 9 * 0.5: a new surface");
  r = tm_fuse(true, 7.f, 0.5f, true, 4.f, 0.5f, 7, 9.f);            // e e = 9 = gate2 s exactly
  CHECK(r.disp == 5.5f && r.var == 0.25f && r.age == 7, "the gate is inclusive");
  r = tm_fuse(true, 60.f, 0.25f, true, 4.f, 0.25f, 255, kInf);
  CHECK(r.disp == 32.f && r.age == 255, "the gate switched off");
  CHECK(tm_pred_ok(1.f, 0.f, kInf) && !tm_pred_ok(0.f, 0.1f, kInf) && !tm_pred_ok(1.f, 2.f, 1.f) && !tm_pred_ok(1.f, kNan, kInf) &&
            !tm_pred_ok(kNan, 1.f, kInf) && !tm_pred_ok(1.f, -1.f, kInf),
        "p_ok");
  CHECK(tm_meas_ok(1.f, 0.25f, 0.0625f) && !tm_meas_ok(kNan, 0.25f, 0.0625f) && !tm_meas_ok(kInf, 0.25f, 0.0625f) &&
            !tm_meas_ok(0.f, 0.25f, 0.0625f) && !tm_meas_ok(1.f, 0.f, 0.0625f) && !tm_meas_ok(1.f, kInf, 0.0625f) &&
            !tm_meas_ok(1.f, kNan, 0.0625f),
        "m_ok");
}

}  // namespace

int main() {
  check_identity();
  check_refused_pixels();
  check_key_order();
  check_payload();
  check_fuse();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
