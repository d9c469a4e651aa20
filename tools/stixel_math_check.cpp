// Host check of the stixel arithmetic (csrc/stixel_math.h, the text the kernels of csrc/stixel.hip compile): the recursion,
// driven serially through sx_relax, against a brute force of its own -- every segmentation and every labelling of small
// columns, the energy written out from the definition of include/dca_hip.h -- and the pieces: the rank selection against a
// sort, the rounded mean against exact rationals, the object term against the sum of squared deviations at the largest
// values the limits allow, the key's order and round trip, the clamp of the road's disparity.  Plain C++, no device, no HIP
// header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <package>/csrc \
//       tools/stixel_math_check.cpp -o stixel_check && ./stixel_check
// Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "stixel_math.h"

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

SxParams defaults() {
  return SxParams{1024, 1024, 16, 2048, 512, 16, 2048, {256, 384, 256}, {0, 0, 0}, {{-1, 0, 0}, {0, 0, 0}, {-1, -1, -1}}};
}

struct Seg {
  int kb, kt, c;
};

// the recursion as the kernel runs it, one candidate at a time: cost[c][k + 1] = cost of the cells [0, k] with top class c
long long solve(const std::vector<int>& q, const std::vector<int>& g, const SxParams& P, std::vector<Seg>* segs) {
  const int H = (int)q.size();
  std::vector<int> N(H + 1, 0), S1(H + 1, 0);
  std::vector<long long> S2(H + 1, 0), G(H + 1, 0), K(H + 1, 0);
  for (int k = 0; k < H; ++k) {
    const bool v = q[k] >= 0;
    N[k + 1] = N[k] + (v ? 1 : 0), S1[k + 1] = S1[k] + (v ? q[k] : 0), S2[k + 1] = S2[k] + (v ? (long long)q[k] * q[k] : 0);
    G[k + 1] = G[k] + (v ? sx_ground_term(q[k], g[k], P.Tg) : 0u), K[k + 1] = K[k] + (v ? sx_sky_term(q[k], P.Ts) : 0u);
  }
  std::vector<long long> C[3] = {std::vector<long long>(H + 1, 0), std::vector<long long>(H + 1, 0), std::vector<long long>(H + 1, 0)};
  std::vector<int> back[3] = {std::vector<int>(H, 0), std::vector<int>(H, 0), std::vector<int>(H, 0)};
  std::vector<unsigned long long> open(4 * H);               // sx_open of every kb, formed once the cells below it are done
  for (int kt = 0; kt < H; ++kt) {
    const long long prev[3] = {C[0][kt], C[1][kt], C[2][kt]};
    sx_open(P, kt, prev, &open[4 * kt]);
    unsigned long long key[3] = {SX_NO_KEY, SX_NO_KEY, SX_NO_KEY};
    for (int kb = 0; kb <= kt; ++kb)
      sx_relax(P, N[kt + 1] - N[kb], S1[kt + 1] - S1[kb], S2[kt + 1] - S2[kb], G[kt + 1] - G[kb], K[kt + 1] - K[kb], g[kb],
               &open[4 * kb], key);
    for (int c = 0; c < 3; ++c) {
      CHECK(key[c] < SX_NO_WAY, "a single segment is never forbidden");
      C[c][kt + 1] = sx_key_cost(key[c]), back[c][kt] = (int)(key[c] & 0xfff);
    }
  }
  int c = sx_top_class(C[0][H], C[1][H], C[2][H]);
  const long long energy = C[c][H];
  segs->clear();
  for (int kt = H - 1;;) {
    const int kb = back[c][kt] >> 2, cp = back[c][kt] & 3;
    segs->push_back({kb, kt, c});
    if (kb == 0) break;
    CHECK(cp < 3 && kb <= kt, "a back-pointer above the bottom names a class");
    kt = kb - 1, c = cp;
  }
  std::reverse(segs->begin(), segs->end());
  return energy;
}

// the energy of one labelled segmentation, from the definition; -1 if a pair is forbidden
long long energy_of(const std::vector<int>& q, const std::vector<int>& g, const SxParams& P, const std::vector<Seg>& segs) {
  long long e = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    const Seg& s = segs[i];
    long long n = 0, sum = 0;
    for (int k = s.kb; k <= s.kt; ++k)
      if (q[k] >= 0) n += 1, sum += q[k];
    const long long mu = n ? (2 * sum + n) / (2 * n) : -1;
    for (int k = s.kb; k <= s.kt; ++k) {
      if (q[k] < 0) continue;
      const long long v = q[k];
      if (s.c == 0) e += std::min((v - g[k]) * (v - g[k]), (long long)P.Tg);
      if (s.c == 1) e += (v - mu) * (v - mu);
      if (s.c == 2) e += std::min(v * v, (long long)P.Ts);
    }
    e += P.seg[s.c];
    if (s.c == 1 && mu >= 0 && mu < P.mu_min) e += P.far;
    if (i == 0) {
      e += P.first[s.c];
      continue;
    }
    const int cp = segs[i - 1].c;
    if (P.T[cp][s.c] < 0) return -1;
    e += P.T[cp][s.c];
    if (s.c == 1 && cp == 0) {
      if (mu > g[s.kb] + P.eps) e += P.below;
      else if (mu < g[s.kb] - P.eps) e += P.hang;
    }
  }
  return e;
}

long long brute(const std::vector<int>& q, const std::vector<int>& g, const SxParams& P) {
  const int H = (int)q.size();
  long long best = -1;
  for (unsigned cuts = 0; cuts < (1u << (H - 1)); ++cuts) {       // bit k: a cut above cell k
    std::vector<Seg> segs;
    int kb = 0;
    for (int k = 0; k < H; ++k)
      if (k == H - 1 || (cuts >> k & 1)) segs.push_back({kb, k, 0}), kb = k + 1;
    int labellings = 1;
    for (size_t i = 0; i < segs.size(); ++i) labellings *= 3;
    for (int l = 0; l < labellings; ++l) {
      int r = l;
      for (Seg& s : segs) s.c = r % 3, r /= 3;
      const long long e = energy_of(q, g, P, segs);
      if (e >= 0 && (best < 0 || e < best)) best = e;
    }
  }
  return best;
}

void check_recursion() {
  std::vector<Seg> segs;
  for (int trial = 0; trial < 400; ++trial) {
    const int H = 1 + trial % 7;
    std::vector<int> q(H), g(H);
    for (int k = 0; k < H; ++k) q[k] = rnd() % 5 == 0 ? -1 : rnd_in(0, 200), g[k] = rnd_in(-50, 200);
    SxParams P = defaults();
    if (trial % 4 == 1) P.first[0] = 7, P.first[1] = 300, P.first[2] = 0, P.T[1][1] = 40, P.T[0][2] = 3, P.T[2][1] = 900;
    if (trial % 4 == 2) P.Tg = 50, P.Ts = 70, P.eps = 0, P.mu_min = 100, P.far = 33, P.T[0][0] = 5;
    if (trial % 4 == 3) P.seg[0] = P.seg[1] = P.seg[2] = 0, P.below = 1, P.hang = 2;
    const long long e = solve(q, g, P, &segs), want = brute(q, g, P);
    CHECK(e == want, "trial %d H %d: recursion %lld, brute force %lld", trial, H, e, want);
    CHECK(energy_of(q, g, P, segs) == e, "trial %d: the segmentation returned has the energy returned", trial);
    CHECK(segs.front().kb == 0 && segs.back().kt == H - 1, "it covers the column");
    for (size_t i = 1; i < segs.size(); ++i) CHECK(segs[i].kb == segs[i - 1].kt + 1, "segments are adjacent");
  }
  // a tie: with nothing to pay, every segmentation of an all-invalid column costs 0 -- the smallest kb wins: ONE segment,
  // and the smallest class
  SxParams P = defaults();
  P.seg[0] = P.seg[1] = P.seg[2] = 0, P.hang = P.below = 0;
  std::vector<int> q(6, -1), g(6, 100);
  CHECK(solve(q, g, P, &segs) == 0 && segs.size() == 1 && segs[0].c == 0, "tie: %zu segments, class %d", segs.size(), segs[0].c);
  // the largest column the limits allow, alternating extremes: every total stays in range and is what the definition gives
  q.assign(1024, 0), g.assign(1024, -16384);
  for (int k = 0; k < 1024; ++k) q[k] = (k & 1) ? 16383 : 0;
  P = defaults();
  P.Tg = P.Ts = SX_MAX_CONST;
  const long long e = solve(q, g, P, &segs);
  CHECK(e > 0 && e < (1LL << 39) && energy_of(q, g, P, segs) == e, "the largest column: %lld", e);
}

void check_pieces() {
  // the rounded mean: |2 n mu - 2 s1| <= n, ties up
  for (int n = 1; n <= 9; ++n)
    for (int s1 = 0; s1 <= 40; ++s1) {
      const int mu = sx_mu(n, s1);
      CHECK(2 * n * mu - 2 * s1 <= n && 2 * s1 - 2 * n * mu < n, "mu %d of %d / %d", mu, s1, n);
    }
  CHECK(sx_mu(0, 0) == -1 && sx_mu(1024, 1024 * 16383) == 16383 && sx_mu(2, 1) == 1, "mean: none, the largest, a tie");
  // the object term is the sum of squared deviations from mu, also at the largest values
  const int n = 1024, s1 = 512 * 16383;
  const long long s2 = 512LL * 16383 * 16383;
  const int mu = sx_mu(n, s1);
  long long want = 0;
  for (int k = 0; k < n; ++k) want += (long long)(((k & 1) ? 16383 : 0) - mu) * (((k & 1) ? 16383 : 0) - mu);
  CHECK(sx_object_cost(n, s1, s2, mu) == want && want < (1LL << 38), "object term %lld", want);
  CHECK(sx_object_cost(0, 0, 0, -1) == 0, "no cell, no cost");
  CHECK(sx_ground_term(0, -16384, SX_MAX_CONST) == (unsigned)SX_MAX_CONST && sx_ground_term(16383, -16384, 1 << 30) == 32767u * 32767u,
        "ground term truncated");
  CHECK(sx_ground_term(100, 97, 1024) == 9 && sx_sky_term(5, 1024) == 25 && sx_sky_term(16383, 1024) == 1024, "terms");
  // the key: order and round trip
  CHECK(sx_key(5, 9, 2) < sx_key(6, 0, 3) && sx_key(5, 3, 2) < sx_key(5, 4, 0) && sx_key(5, 3, 0) < sx_key(5, 3, 1), "key order");
  const unsigned long long key = sx_key((1LL << 50) - 1, 1023, 3);
  CHECK(sx_key_cost(key) == (1LL << 50) - 1 && sx_key_kb(key) == 1023 && sx_key_cp(key) == 3 && key < SX_NO_WAY, "key round trip");
  CHECK(sx_key(7, 5, 2) + (9ull << 12) == sx_key(16, 5, 2) && SX_NO_WAY + ((1ull << 39) << 12) < SX_NO_KEY, "a key is linear in its cost");
  CHECK(sx_top_class(4, 4, 4) == 0 && sx_top_class(5, 4, 4) == 1 && sx_top_class(5, 5, 4) == 2, "top class");
  // rank selection against a sort
  for (int trial = 0; trial < 200; ++trial) {
    const int m = rnd_in(1, 129), nbits = sx_value_bits(rnd_in(8, 1025));
    std::vector<int> v(m);
    for (int& x : v) x = rnd_in(0, trial % 3 ? 1 << nbits : 4);
    std::vector<int> sorted = v;
    std::sort(sorted.begin(), sorted.end());
    const int rank = (m - 1) / 2;
    const int got = sx_rank_select(nbits, rank, [&](int t) {
      int c = 0;
      for (int x : v) c += x < t;
      return c;
    });
    CHECK(got == sorted[rank], "rank %d of %d: %d, sorted %d", rank, m, got, sorted[rank]);
  }
  CHECK(sx_value_bits(8) == 7 && sx_value_bits(192) == 12 && sx_value_bits(1024) == 14, "bits");
  // the road's disparity: rounding, clamps, NaN and infinities
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(sx_ground_q(0.f, 0.f, 2.5f, 0, 0, 32) == 40 && sx_ground_q(0.f, 0.f, -0.03125f, 0, 0, 32) == 0, "rounding");
  CHECK(sx_ground_q(0.f, 0.f, -0.04f, 0, 0, 32) == -1 && sx_ground_q(0.5f, 0.25f, 3.0f, -4, 8, 32) == 48, "rounding");
  CHECK(sx_ground_q(0.f, 0.f, 1e30f, 0, 0, 32) == 512 && sx_ground_q(0.f, 0.f, -1e30f, 0, 0, 32) == -512, "clamps");
  CHECK(sx_ground_q(0.f, 0.f, inf, 0, 0, 32) == 512 && sx_ground_q(0.f, 0.f, -inf, 0, 0, 32) == -512, "infinities");
  CHECK(sx_ground_q(nan, 0.f, 0.f, 1, 0, 1024) == -16384, "a NaN goes to the lower end");
  // the grid: cell 0 at the bottom, leftovers at the top; the centre
  CHECK(sx_cell_row0(0, 11, 2) == 9 && sx_cell_row0(4, 11, 2) == 1 && sx_centre_row(0, 11, 2) == 10 && sx_centre_row(3, 10, 1) == 6,
        "rows");
  CHECK(sx_centre_col(0, 5) == 2 && sx_centre_col(3, 4) == 14 && sx_centre_col(7, 1) == 7, "columns");
  const SxParams P = defaults();
  CHECK(sx_far(P, -1) == 0 && sx_far(P, 0) == 2048 && sx_far(P, 15) == 2048 && sx_far(P, 16) == 0, "far");
  CHECK(sx_contact(P, 117, 100) == 2048 && sx_contact(P, 116, 100) == 0 && sx_contact(P, 84, 100) == 0 && sx_contact(P, 83, 100) == 512,
        "contact");
}

}  // namespace

int main() {
  check_recursion();
  check_pieces();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
