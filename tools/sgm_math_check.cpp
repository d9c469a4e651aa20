// Host check of the arithmetic of semi-global matching (csrc/sgm_math.h, the text the kernels of csrc/sgm.hip compile): the
// recursion step, driven along whole paths, against the formula of include/dca_hip.h written out with its conditions; its bounds
// C <= L_r <= C + P2 and S < 65536 at the extremes (P1 = P2 = 4095, cost 62, 8 paths); the uniqueness test against the
// definition bin by bin; the sub-pixel step against rounding half up in exact integers, exhaustively over small inputs and at the
// largest values S can take; the grey value.  Plain C++, no device, no HIP header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <package>/csrc \
//       tools/sgm_math_check.cpp -o sgm_check && ./sgm_check
// Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sgm_math.h"

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

unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
unsigned rnd() {                                             // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (unsigned)((rng_state * 0x2545f4914f6cdd1dull) >> 33);
}
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo)); }      // [lo, hi)

const int S_MAX = 8 * (SGM_COST_OUT + SGM_MAX_P);            // 33256

// the definition, with its conditions spelled out
int step_by_definition(const std::vector<int>& prev, int d, int c, int P1, int P2) {
  const int D = (int)prev.size();
  const int m = *std::min_element(prev.begin(), prev.end());
  long long best = prev[d];
  if (d >= 1) best = std::min<long long>(best, (long long)prev[d - 1] + P1);
  if (d <= D - 2) best = std::min<long long>(best, (long long)prev[d + 1] + P1);
  best = std::min<long long>(best, (long long)m + P2);
  return (int)(c + best - m);
}

// one path of `steps` pixels over D bins through sgm_step, as a kernel's lanes drive it; returns the largest L seen
int drive_path(int D, int steps, int P1, int P2, int cost_kind) {
  std::vector<int> prev(D), cur(D), c(D);
  int largest = 0;
  for (int t = 0; t < steps; ++t) {
    for (int d = 0; d < D; ++d) {
      switch (cost_kind) {
        case 0: c[d] = rnd_in(0, SGM_COST_OUT + 1); break;
        case 1: c[d] = rnd() & 1 ? SGM_COST_OUT : 0; break;                    // the two ends only
        case 2: c[d] = SGM_COST_OUT; break;
        default: c[d] = d == (t < steps / 2 ? 0 : D - 1) ? 0 : SGM_COST_OUT; break;      // one cheap bin for long, then another
      }
    }
    if (t == 0) {
      cur = c;
    } else {
      const int m = *std::min_element(prev.begin(), prev.end());
      for (int d = 0; d < D; ++d) {
        const int lm = d >= 1 ? prev[d - 1] : SGM_NONE, lp = d <= D - 2 ? prev[d + 1] : SGM_NONE;
        cur[d] = sgm_step(c[d], prev[d], lm, lp, m, P1, P2);
        const int want = step_by_definition(prev, d, c[d], P1, P2);
        CHECK(cur[d] == want, "step D=%d t=%d d=%d P=(%d,%d): %d, by definition %d", D, t, d, P1, P2, cur[d], want);
      }
    }
    for (int d = 0; d < D; ++d) {
      CHECK(cur[d] >= c[d] && cur[d] <= c[d] + P2, "bound D=%d t=%d d=%d: C %d L %d P2 %d", D, t, d, c[d], cur[d], P2);
      largest = std::max(largest, cur[d]);
    }
    prev = cur;
  }
  return largest;
}

void check_recursion() {
  // exhaustive small inputs: D = 2 and 3, every previous row and every cost out of a few values, a few penalties
  const int vals[4] = {0, 1, 5, SGM_COST_OUT};
  const int pens[4][2] = {{1, 1}, {1, 3}, {2, 2}, {10, 120}};
  for (int D = 2; D <= 3; ++D) {
    int n = 1;
    for (int i = 0; i < D; ++i) n *= 4;
    for (int code = 0; code < n; ++code) {
      std::vector<int> prev(D);
      for (int i = 0, k = code; i < D; ++i, k /= 4) prev[i] = vals[k % 4] + (i == 1 ? 3 : 0);
      const int m = *std::min_element(prev.begin(), prev.end());
      for (const auto& p : pens)
        for (int c : vals)
          for (int d = 0; d < D; ++d) {
            const int lm = d >= 1 ? prev[d - 1] : SGM_NONE, lp = d <= D - 2 ? prev[d + 1] : SGM_NONE;
            const int got = sgm_step(c, prev[d], lm, lp, m, p[0], p[1]);
            CHECK(got == step_by_definition(prev, d, c, p[0], p[1]), "exhaustive D=%d code=%d d=%d", D, code, d);
            CHECK(got >= c && got <= c + p[1], "exhaustive bound D=%d code=%d d=%d", D, code, d);
          }
    }
  }
  // whole paths, random and adversarial costs, the extremes of the penalties included
  int largest = 0;
  for (int kind = 0; kind < 4; ++kind)
    for (const int D : {1, 2, 3, 8, 24, 256}) {
      if (D == 1) {                                          // (the operator starts at 8 bins; one bin: both neighbours missing)
        const int got = sgm_step(7, 9, SGM_NONE, SGM_NONE, 9, SGM_MAX_P, SGM_MAX_P);
        CHECK(got == 7, "one bin: %d", got);
        continue;
      }
      drive_path(D, 200, 10, 120, kind);
      drive_path(D, 200, 1, 1, kind);
      drive_path(D, 200, 1, SGM_MAX_P, kind);
      largest = std::max(largest, drive_path(D, 400, SGM_MAX_P, SGM_MAX_P, kind));
    }
  CHECK(largest <= SGM_COST_OUT + SGM_MAX_P, "the largest L_r: %d", largest);
  CHECK(8 * largest < 65536 && S_MAX < 65536 && 8 * largest <= S_MAX, "8 paths: %d", 8 * largest);
  CHECK(largest == SGM_COST_OUT + SGM_MAX_P, "the adversarial costs reach the bound itself: %d", largest);
  CHECK(SGM_NONE > S_MAX && (long long)SGM_NONE + SGM_MAX_P < 2147483647LL && (long long)SGM_NONE * 100 < 2147483647LL,
        "SGM_NONE is above every value and its uses stay an int");
}

void check_uniqueness() {
  const int us[6] = {0, 1, 15, 50, 98, 99};
  for (int trial = 0; trial < 4000; ++trial) {
    const int D = rnd_in(4, 12), top = trial % 3 == 0 ? S_MAX + 1 : (trial % 3 == 1 ? 60 : 1000);
    std::vector<int> S(D);
    for (int& v : S) v = rnd_in(trial % 7 == 0 ? top - std::min(top, 5) : 0, top);
    const int ds = (int)(std::min_element(S.begin(), S.end()) - S.begin()), s = S[ds];      // the lowest index of the minimum
    int other = SGM_NONE;
    for (int k = 0; k < D; ++k)
      if (k < ds - 1 || k > ds + 1) other = sgm_min(other, S[k]);
    for (int u : us) {
      bool want = true;
      for (int k = 0; k < D; ++k)
        if (std::abs(k - ds) > 1) want = want && (long long)S[k] * (100 - u) >= 100LL * s;
      CHECK(sgm_unique(s, other, u) == want, "trial %d u=%d s=%d other=%d", trial, u, s, other);
      if (u == 0) CHECK(sgm_unique(s, other, 0), "u = 0 switches the test off: s=%d other=%d", s, other);
    }
  }
  CHECK(sgm_unique(S_MAX, S_MAX, 0) && !sgm_unique(S_MAX, S_MAX, 1) && sgm_unique(0, 0, 99) && !sgm_unique(100, 100, 1) && sgm_unique(99, 100, 1), "edges");
}

long long floor_div(long long a, long long b) {              // b > 0
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

void check_one_subpixel(int sm, int s, int sp) {
  const int off = sgm_subpixel(sm, s, sp), den = sm + sp - 2 * s;
  if (den <= 0) {
    CHECK(off == 0, "den = 0: %d", off);
    return;
  }
  CHECK(16 * (sm - sp) + 17 * den >= den, "the numerator is at least den: sm=%d s=%d sp=%d", sm, s, sp);
  const long long want = floor_div(2LL * 8 * (sm - sp) + den, 2LL * den);      // floor(8 (sm - sp) / den + 1/2)
  CHECK(off == want, "sm=%d s=%d sp=%d: %d, rounded half up %lld", sm, s, sp, off, want);
  CHECK(off >= -8 && off <= 8, "sm=%d s=%d sp=%d: %d outside [-8, 8]", sm, s, sp, off);
}

void check_subpixel() {
  for (int s = 0; s <= 12; ++s)
    for (int sm = s; sm <= s + 70; ++sm)
      for (int sp = s; sp <= s + 70; ++sp) check_one_subpixel(sm, s, sp);
  for (int trial = 0; trial < 20000; ++trial) {
    const int s = rnd_in(0, S_MAX + 1);
    check_one_subpixel(rnd_in(s, S_MAX + 1), s, rnd_in(s, S_MAX + 1));
  }
  check_one_subpixel(S_MAX, 0, 0), check_one_subpixel(0, 0, S_MAX), check_one_subpixel(S_MAX, 0, S_MAX);
  check_one_subpixel(S_MAX, S_MAX, S_MAX), check_one_subpixel(S_MAX, S_MAX - 1, S_MAX);
  CHECK(sgm_subpixel(10, 0, 0) == 8 && sgm_subpixel(0, 0, 10) == -8 && sgm_subpixel(5, 0, 5) == 0 && sgm_subpixel(3, 3, 3) == 0,
        "the ends and the middle");
  CHECK(sgm_subpixel(9, 0, 7) == 1 && sgm_subpixel(7, 0, 9) == -1 && sgm_subpixel(9, 0, 8) == 0 && sgm_subpixel(8, 0, 9) == 0,
        "8 * 2 / 16 = 1, 8 * -2 / 16 = -1, 8 / 17 and -8 / 17 round to 0: %d %d", sgm_subpixel(9, 0, 7), sgm_subpixel(7, 0, 9));
}

void check_grey() {
  for (int v = 0; v < 256; ++v) CHECK(sgm_grey(v, v, v) == v, "grey stays grey: %d -> %d", v, sgm_grey(v, v, v));
  for (int r = 0; r < 256; r += 5)
    for (int g = 0; g < 256; g += 3)
      for (int b = 0; b < 256; b += 17) {
        const int y = sgm_grey(r, g, b);
        CHECK(y >= 0 && y <= 255 && y == (77 * r + 150 * g + 29 * b + 128) / 256, "grey(%d,%d,%d) = %d", r, g, b, y);
      }
  CHECK(sgm_grey(255, 255, 255) == 255 && sgm_grey(0, 0, 0) == 0 && sgm_grey(255, 0, 0) == 77 && sgm_grey(0, 255, 0) == 149, "corners");
}

}  // namespace

int main() {
  check_recursion();
  check_uniqueness();
  check_subpixel();
  check_grey();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
