// Host check of the ground-plane arithmetic (csrc/ground_math.h, the text the kernels of csrc/ground.hip compile): the floor
// division and the line's bin against exact rational arithmetic for negative numerators and at every boundary bin, the
// Hough key's order and its round trip, the validity test at its edges, and the 3x3 solve on singular, rank-2 and
// well-conditioned sums.  Plain C++, no device, no HIP header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <package>/csrc \
//       tools/ground_math_check.cpp -o ground_check && ./ground_check
// Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ground_math.h"

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

// floor(a / b) by search, b > 0: the largest q with q b <= a
long long floor_div_ref(long long a, long long b) {
  long long q = a / b;
  while (q * b > a) --q;
  while ((q + 1) * b <= a) ++q;
  return q;
}

void check_floor_div() {
  for (int b : {1, 2, 3, 7, 78, 2 * 32767}) {
    for (int a = -300; a <= 300; ++a) CHECK(gm_floor_div(a, b) == floor_div_ref(a, b), "a %d b %d", a, b);
    for (int k = -5; k <= 5; ++k)
      for (int e = -1; e <= 1; ++e) {
        const long long a = (long long)k * b + e;
        CHECK(gm_floor_div((int)a, b) == floor_div_ref(a, b), "a %lld b %d", a, b);
      }
  }
  const int big = (1 << 27) - 1;                              // the largest numerator the limits allow
  CHECK(gm_floor_div(big, 2 * 32767) == floor_div_ref(big, 2 * 32767), "large positive");
  CHECK(gm_floor_div(-big, 2 * 32767) == floor_div_ref(-big, 2 * 32767), "large negative");
}

// the line's bin is floor(line(r) + 1/2) in exact arithmetic, for every candidate of the range at the window's first, middle
// and last rows, including d_top = -NB, d_top = NB - 1, d_bot = 1 and d_bot = NB - 1
void check_line_bin() {
  for (int R : {2, 3, 40, 53, 32768})
    for (int NB : {8, 32, 1024}) {
      const int tops[] = {-NB, -NB + 1, -1, 0, 1, NB - 1}, bots[] = {1, 2, NB / 2, NB - 1};
      const int rows[] = {0, 1, R / 2, R - 2 < 0 ? 0 : R - 2, R - 1};
      for (int d_top : tops)
        for (int d_bot : bots)
          for (int r : rows) {
            const long long num = 2LL * ((long long)d_top * (R - 1 - r) + (long long)d_bot * r) + (R - 1);
            const long long want = floor_div_ref(num, 2LL * (R - 1));
            CHECK(gm_line_bin(d_top, d_bot, r, R) == want, "R %d NB %d top %d bot %d r %d", R, NB, d_top, d_bot, r);
            if (r == 0) CHECK(gm_line_bin(d_top, d_bot, r, R) == d_top, "row 0 is d_top");
            if (r == R - 1) CHECK(gm_line_bin(d_top, d_bot, r, R) == d_bot, "row R-1 is d_bot");
          }
    }
  // a line through zero: -1/2 rounds to bin 0 (floor(-1/2 + 1/2) = 0), just below it to -1
  CHECK(gm_line_bin(-1, 0, 1, 3) == 0, "half below zero");        // line(1) = -1/2
  CHECK(gm_line_bin(-2, 1, 1, 4) == -1, "line(1) = -1");
  CHECK(gm_line_bin(-3, 1, 1, 5) == -2, "line(1) = -2");
}

void check_key() {
  for (int NB : {8, 192, 1024}) {
    int v, t, b;
    for (int d_bot : {1, 2, NB - 1})
      for (int d_top : {-NB, -1, 0, NB - 1})
        for (int vote : {0, 1, 12345, std::numeric_limits<int>::max()}) {
          const unsigned long long k = gm_hough_key(vote, d_top, d_bot, NB);
          CHECK(k != 0, "a key is never zero");
          gm_hough_unkey(k, NB, &v, &t, &b);
          CHECK(v == vote && t == d_top && b == d_bot, "round trip NB %d", NB);
        }
    CHECK(gm_hough_key(5, 0, 3, NB) > gm_hough_key(4, -NB, 1, NB), "the larger vote wins");
    CHECK(gm_hough_key(5, NB - 1, 2, NB) > gm_hough_key(5, -NB, 3, NB), "then the smaller d_bot");
    CHECK(gm_hough_key(5, -2, 3, NB) > gm_hough_key(5, -1, 3, NB), "then the smaller d_top");
  }
}

void check_valid() {
  int q = -1;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float bad : {nan, inf, -inf, -1.0f, 0.0f, 0.06f, 32.0f, 31.97f, 1e30f, 3e38f})
    CHECK(!gm_valid(bad, 0.0625f, 32, &q), "%g must not be valid", (double)bad);
  CHECK(gm_valid(0.0625f, 0.0625f, 32, &q) && q == 1, "min_disp itself");
  CHECK(gm_valid(31.96f, 0.0625f, 32, &q) && q == 511 && (q >> 4) == 31, "the last bin, q %d", q);
  CHECK(gm_valid(-0.0f, 0.0f, 8, &q) && q == 0, "-0.0 with min_disp 0");
  CHECK(gm_valid(1023.96f, 0.0f, 1024, &q) && (q >> 4) == 1023, "the last bin of the largest NB");
  CHECK(!gm_valid(1024.0f, 0.0f, 1024, &q), "NB itself");
}

struct Pt {
  int u, v, q;
};

void sums_of(const std::vector<Pt>& pts, long long* S) {
  for (int i = 0; i < GM_SUMS; ++i) S[i] = 0;
  for (const Pt& p : pts) {
    const long long u = p.u, v = p.v, q = p.q;
    S[GM_N] += 1, S[GM_SU] += u, S[GM_SV] += v, S[GM_SQ] += q, S[GM_SUU] += u * u, S[GM_SUV] += u * v, S[GM_SVV] += v * v;
    S[GM_SUQ] += u * q, S[GM_SVQ] += v * q, S[GM_SQQ] += q * q;
  }
}

void check_solve() {
  long long S[GM_SUMS];
  double fit[4] = {-1, -1, -1, -1};
  // singular: no point; one point; one column (u constant); one row (v constant); points on one line in (u, v)
  std::vector<Pt> pts;
  sums_of(pts, S);
  CHECK(!gm_solve(S, fit), "no point");
  pts = {{3, 4, 100}};
  sums_of(pts, S);
  CHECK(!gm_solve(S, fit), "one point");
  pts.clear();
  for (int v = -10; v < 10; ++v) pts.push_back({7, v, 160 + 8 * v});
  sums_of(pts, S);
  CHECK(!gm_solve(S, fit), "one column: rank 2");
  pts.clear();
  for (int u = -30; u < 30; ++u) pts.push_back({u, -5, 160 + u});
  sums_of(pts, S);
  CHECK(!gm_solve(S, fit), "one row: rank 2");
  pts.clear();
  for (int k = -20; k < 20; ++k) pts.push_back({2 * k, 3 * k, 200 + k});
  sums_of(pts, S);
  CHECK(!gm_solve(S, fit), "a diagonal: rank 2");
  CHECK(std::isfinite(fit[0]) && std::isfinite(fit[1]) && std::isfinite(fit[2]) && fit[3] >= 0.0,
        "a refused solve leaves finite numbers (the caller drops them)");
  // well conditioned, exact data q = 16 (a u + b v + c) with a = 1/8, b = 1/2, c = 10: recovered to rounding, rms 0
  pts.clear();
  for (int v = -12; v < 12; ++v)
    for (int u = -37; u < 38; ++u) pts.push_back({u, v, 2 * u + 8 * v + 160});
  sums_of(pts, S);
  CHECK(gm_solve(S, fit), "a plane");
  CHECK(std::fabs(fit[0] - 0.125) < 1e-12 && std::fabs(fit[1] - 0.5) < 1e-12 && std::fabs(fit[2] - 10.0) < 1e-10,
        "a %.17g b %.17g c %.17g", fit[0], fit[1], fit[2]);
  CHECK(fit[3] >= 0.0 && fit[3] < 1e-5, "rms %.17g", fit[3]);
  // the same with a residual of +-1 sixteenth in a checkerboard: rms close to 1/16 px, never negative or NaN
  for (Pt& p : pts) p.q += ((p.u + p.v) & 1) ? 1 : -1;
  sums_of(pts, S);
  CHECK(gm_solve(S, fit), "a noisy plane");
  CHECK(std::fabs(fit[3] - 1.0 / 16.0) < 1e-3 && std::fabs(fit[1] - 0.5) < 1e-3, "rms %.17g b %.17g", fit[3], fit[1]);
  // a KITTI-sized frame at the largest coordinates: sums of 2^40 and products beyond 2^53 stay finite and accurate
  pts.clear();
  for (int v = 0; v < 192; v += 3)
    for (int u = -624; u < 624; u += 5) pts.push_back({u, v, 16 * 40 + 5 * v + u / 64});
  sums_of(pts, S);
  CHECK(gm_solve(S, fit) && std::isfinite(fit[0]) && std::fabs(fit[1] - 5.0 / 16.0) < 1e-3, "large frame b %.17g", fit[1]);
  // the pose of a level road: hs = baseline / b, the normal straight down
  double hs_n[4];
  gm_pose(0.0, 1.0 / 3.0, 0.0, 37.0, 24.0, 60.0, 0.5, 37.0, 24.0, 0.0, 0.0, hs_n);
  CHECK(std::fabs(hs_n[0] - 1.5) < 1e-12 && hs_n[1] == 0.0 && std::fabs(hs_n[2] - 1.0) < 1e-12 && std::fabs(hs_n[3]) < 1e-12,
        "pose %.17g %.17g %.17g %.17g", hs_n[0], hs_n[1], hs_n[2], hs_n[3]);
  gm_pose(0.0, 0.0, 0.0, 0.0, 0.0, 60.0, 0.5, 0.0, 0.0, 0.0, 0.0, hs_n);
  CHECK(hs_n[0] == 0.0 && hs_n[2] == 0.0, "no plane, no pose");
  double b, c;
  gm_line_plane(-32, 30, 40, &b, &c);
  CHECK(b == 62.0 / 39.0 && c == -32.0 + b * 20.0, "the Hough line as a plane");
  CHECK(gm_line_disp(-32, 30, 0, 40) == -32.0f && gm_line_disp(-32, 30, 39, 40) == 30.0f, "the line's ends");
  CHECK(gm_plane_disp(0.5f, 0.25f, 3.0f, -4, 8) == 3.0f, "the plane");
}

}  // namespace

int main() {
  check_floor_div();
  check_line_bin();
  check_key();
  check_valid();
  check_solve();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
