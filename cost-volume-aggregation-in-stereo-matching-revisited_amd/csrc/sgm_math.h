// The arithmetic of semi-global matching (include/dca_hip.h, dca_sgm_disparity), written ONCE for the kernels of sgm.hip and for
// the host check tools/sgm_math_check.cpp: the grey value, one step of the path recursion, the uniqueness test and the sub-pixel
// step.  Integers only.
//
// Bounds.  C <= 62, 1 <= P1 <= P2 <= SGM_MAX_P = 4095.  By induction C <= L_r <= C + P2: the minimum of the four terms is at
// least m (every term is) and at most m + P2 (the last one).  So L_r <= 4157, the sum of 8 paths <= 33256 < 2^16, and an int
// holds every intermediate, SGM_NONE + P1 included.
#pragma once

#if defined(__HIPCC__)
#define SGM_HD __host__ __device__ inline
#else
#define SGM_HD inline
#endif

#define SGM_MAX_P 4095
#define SGM_COST_OUT 62
#define SGM_NONE (1 << 20)           // "no such bin": above every L_r, and SGM_NONE + P1 stays an int; never wins a minimum

SGM_HD int sgm_min(int a, int b) { return a < b ? a : b; }

// (77 R + 150 G + 29 B + 128) >> 8: the weights sum to 256, so grey stays grey and the result a byte
SGM_HD int sgm_grey(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

// One step of the recursion for one bin: c = C(p,d); l, lm, lp = L_r(p-r, d), (d-1), (d+1), SGM_NONE for a bin that does not
// exist (d = 0, d = D-1); m = min_k L_r(p-r,k).
SGM_HD int sgm_step(int c, int l, int lm, int lp, int m, int P1, int P2) {
  return c + sgm_min(sgm_min(l, m + P2), sgm_min(lm, lp) + P1) - m;
}

// The uniqueness test, given other = min S(p,k) over the k with |k - d*| > 1 (D >= 8: there is always one):
// S(p,k) (100 - u) >= 100 s holds for every such k iff it holds for the smallest.  u = 0: always true, s being the minimum.
SGM_HD bool sgm_unique(int s, int other, int u) { return other * (100 - u) >= 100 * s; }

// The sub-pixel step in sixteenths from sm = S(d*-1), s = S(d*), sp = S(d*+1), s <= sm and s <= sp: the vertex of the parabola,
// 8 (sm - sp) / den rounded half up.  16 (sm - sp) >= -16 (sp - s) >= -16 den makes the numerator >= den > 0, so the division is
// one of positive integers: C and Python agree.  The result lies in [-8, 8].
SGM_HD int sgm_subpixel(int sm, int s, int sp) {
  const int den = sm + sp - 2 * s;
  if (den <= 0) return 0;
  return (16 * (sm - sp) + 17 * den) / (2 * den) - 8;
}
