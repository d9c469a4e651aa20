// The arithmetic of the stixel world (include/dca_hip.h, dca_stixels), written ONCE for the kernels of stixel.hip and for the
// host check tools/stixel_math_check.cpp: the cell grid and its centre, the ground disparity of a cell, the rank selection
// behind the median, the data terms, the rounded mean of an object, the prior, the packed key and the two halves of one step of
// the recursion (sx_open per bottom cell, sx_relax per bottom and top cell).  Everything but the plane's disparity (ground_math.h) is integer arithmetic in units of 1/16 px and (1/16 px)^2.
//
// Bounds.  q < 2^14 (NB <= 1024), |g| <= 2^14, H <= 1024 cells, every constant of SxParams <= SX_MAX_CONST = 2^20:
//   S1 <= H q < 2^24 (int32),  2 S1 + n < 2^26 (the 32-bit division of the mean),  S2 <= H q^2 < 2^38 (int64),
//   the object term S2 - 2 mu S1 + n mu^2 = sum (q - mu)^2 < 2^38,  a prefix of ground or sky terms <= H 2^20 = 2^30 (uint32),
//   seg + prior of one segment <= 5 2^20 and of at most H segments < 2^33:  every total < 2^39, far below the 2^50 that the key
//   cost << 12 | kb << 2 | cp leaves room for.
#pragma once
#include "ground_math.h"

#define SX_HD GM_HD

#pragma clang fp contract(off)

#define SX_GROUND 0
#define SX_OBJECT 1
#define SX_SKY 2
#define SX_NONE 3                    // "no segment below": the cp of a bottom segment in the key
#define SX_MAX_CONST (1 << 20)
#define SX_NO_KEY (~0ull)

// the constants of the energy, by value; T[cp][c] < 0 forbids class c directly on class cp
struct SxParams {
  int Tg, Ts, eps, below, hang, mu_min, far;
  int seg[3], first[3];
  int T[3][3];
};

// ---- cells: CS = cols / width columns of H = rows / row_step cells, cell 0 at the bottom; what is left over on the right and at
// the top is not covered
SX_HD int sx_cell_row0(int k, int rows, int row_step) { return rows - (k + 1) * row_step; }     // the cell's first (upper) window row
SX_HD int sx_cell_col0(int s, int width) { return s * width; }
// THE centre pixel: the middle one of an odd extent, the lower / right one of the two middle ones of an even extent
SX_HD int sx_centre_row(int k, int rows, int row_step) { return sx_cell_row0(k, rows, row_step) + row_step / 2; }
SX_HD int sx_centre_col(int s, int width) { return sx_cell_col0(s, width) + width / 2; }

// the road's disparity in sixteenths at the centred pixel (u', v'): floorf(p * 16 + 0.5f), clamped to [-16 NB, 16 NB] in float
// before the conversion (a NaN goes to the lower end)
SX_HD int sx_ground_q(float a, float b, float c, int u, int v, int NB) {
  const float t = floorf(gm_plane_disp(a, b, c, u, v) * 16.0f + 0.5f), lim = (float)(16 * NB);
  if (!(t > -lim)) return -16 * NB;
  if (t >= lim) return 16 * NB;
  return (int)t;
}

// bits of the largest quantised disparity 16 NB - 1
SX_HD int sx_value_bits(int NB) {
  int bits = 0;
  for (unsigned v = (unsigned)(16 * NB - 1); v; v >>= 1) ++bits;
  return bits;
}
// the value of rank m (0-based, ascending) among values in [0, 2^nbits), by descent over the bits: count_below(t) = how many
// are < t.  The lower median of n values is rank (n - 1) / 2.  No array, no data-dependent address.
template <class F>
SX_HD int sx_rank_select(int nbits, int m, F count_below) {
  int v = 0;
  for (int bit = 1 << (nbits - 1); bit; bit >>= 1) {
    const int t = v | bit;
    if (count_below(t) <= m) v = t;
  }
  return v;
}

// ---- data terms of one valid cell
SX_HD unsigned sx_ground_term(int q, int g, int Tg) {
  const long long d = (long long)(q - g) * (q - g);
  return (unsigned)(d < Tg ? d : Tg);
}
SX_HD unsigned sx_sky_term(int q, int Ts) {
  const long long d = (long long)q * q;
  return (unsigned)(d < Ts ? d : Ts);
}
// ---- an object over n valid cells with sum s1 and sum of squares s2: the mean rounded to a sixteenth, -1 without a cell
SX_HD int sx_mu(int n, int s1) {
  const unsigned den = n > 0 ? 2u * (unsigned)n : 1u;
  const int mu = (int)((unsigned)(2 * s1 + n) / den);
  return n > 0 ? mu : -1;
}
SX_HD long long sx_object_cost(int n, int s1, long long s2, int mu) {
  const long long c = s2 - 2LL * mu * s1 + (long long)n * mu * mu;
  return n > 0 ? c : 0;
}
// what an object of mean mu pays for itself (far) ...
SX_HD int sx_far(const SxParams& P, int mu) { return (mu >= 0 && mu < P.mu_min) ? P.far : 0; }
// ... and for standing directly on a ground segment, g_kb the road's disparity at its bottom cell; mu is taken as it is
SX_HD int sx_contact(const SxParams& P, int mu, int g_kb) { return mu > g_kb + P.eps ? P.below : (mu < g_kb - P.eps ? P.hang : 0); }

// ---- the key: the unsigned minimum is the smallest cost, then the smallest kb, then the smallest cp (SX_NONE for kb = 0)
SX_HD unsigned long long sx_key(long long cost, int kb, int cp) {
  return (unsigned long long)cost << 12 | (unsigned long long)((unsigned)kb << 2 | (unsigned)cp);
}
SX_HD long long sx_key_cost(unsigned long long key) { return (long long)(key >> 12); }
SX_HD int sx_key_kb(unsigned long long key) { return (int)(key >> 2) & 1023; }
SX_HD int sx_key_cp(unsigned long long key) { return (int)key & 3; }
SX_HD unsigned long long sx_key_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

// ---- the recursion in two halves, so that what does not depend on the segment's top is formed once per kb, not once per
// (kb, kt).  A key is linear in its cost: sx_key(a, kb, cp) + (b << 12) == sx_key(a + b, kb, cp).
// "no way in": above every key, and with any segment's cost << 12 (below 2^51) added still below 2^63
#define SX_NO_WAY (1ull << 62)
// sx_open: what the segmentations of the cells [0, kb) offer a segment that STARTS at cell kb, its own cost left out --
// open[c] = the key of min over cp of prev[cp] + T[cp][c], prev[cp] = cost[kb - 1][cp]; for an object the pair on ground is
// kept apart in open[3], because its contact term depends on the object's mean.  kb = 0: nothing below, first[c] (prev is
// not used).  Straight-line code: the forbidden pairs and kb = 0 are selects.
SX_HD void sx_open(const SxParams& P, int kb, const long long* prev, unsigned long long* open) {
  const bool bottom = kb == 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned long long k = bottom ? sx_key(P.first[c], 0, SX_NONE) : SX_NO_WAY;
#pragma unroll
    for (int cp = 0; cp < 3; ++cp) {
      const int t = P.T[cp][c];
      const bool skip = bottom || t < 0 || (c == SX_OBJECT && cp == SX_GROUND);
      k = sx_key_min(k, skip ? SX_NO_WAY : sx_key(prev[cp] + t, kb, cp));
    }
    open[c] = k;
  }
  const int t = P.T[SX_GROUND][SX_OBJECT];
  open[3] = (bottom || t < 0) ? SX_NO_WAY : sx_key(prev[SX_GROUND] + t, kb, SX_GROUND);
}
// sx_relax: the segment of cells [kb, kt] in every class on what sx_open found for kb.  n, s1, s2: its valid cells; dg, ds:
// its ground and sky terms; g_kb: the road at cell kb.  key[c] takes the minimum.
SX_HD void sx_relax(const SxParams& P, int n, int s1, long long s2, long long dg, long long ds, int g_kb,
                    const unsigned long long* open, unsigned long long* key) {
  const int mu = sx_mu(n, s1);
  const long long ground = dg + P.seg[SX_GROUND], sky = ds + P.seg[SX_SKY];
  const long long object = sx_object_cost(n, s1, s2, mu) + P.seg[SX_OBJECT] + sx_far(P, mu);
  const long long on_ground = object + sx_contact(P, mu, g_kb);
  key[SX_GROUND] = sx_key_min(key[SX_GROUND], open[SX_GROUND] + ((unsigned long long)ground << 12));
  key[SX_OBJECT] = sx_key_min(key[SX_OBJECT], sx_key_min(open[SX_OBJECT] + ((unsigned long long)object << 12),
                                                         open[3] + ((unsigned long long)on_ground << 12)));
  key[SX_SKY] = sx_key_min(key[SX_SKY], open[SX_SKY] + ((unsigned long long)sky << 12));
}

// the class of the top segment: the smallest cost, then the smallest class
SX_HD int sx_top_class(long long c0, long long c1, long long c2) {
  int c = 0;
  long long e = c0;
  if (c1 < e) c = 1, e = c1;
  if (c2 < e) c = 2;
  return c;
}
