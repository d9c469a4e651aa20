// The arithmetic of the ground-plane fit (include/dca_hip.h, dca_ground_plane / dca_ground_segment), written ONCE for the
// kernels of ground.hip and for the host check tools/ground_math_check.cpp: the validity test and the quantisation, the
// floor division and the line's bin, the Hough key, the two predictions, the 3x3 solve and the pose of the plane.
// Every function is the header's formula as it is written, each operation rounded on its own.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GM_HD __host__ __device__ inline
#else
#define GM_HD inline
#endif

#pragma clang fp contract(off)

#define GM_N 0
#define GM_SU 1
#define GM_SV 2
#define GM_SQ 3
#define GM_SUU 4
#define GM_SUV 5
#define GM_SVV 6
#define GM_SUQ 7
#define GM_SVQ 8
#define GM_SQQ 9
#define GM_SUMS 10

// d >= min_disp and its bin below NB -> q, the disparity in sixteenths (0 <= q < 16 NB).  The comparison is made in float
// before the conversion: a NaN and -inf fail the first test, +inf and every d that would overflow an int the second.
GM_HD bool gm_valid(float d, float min_disp, int NB, int* q) {
  if (!(d >= min_disp)) return false;
  const float t = d * 16.0f + 0.5f;
  if (!(t < (float)(16 * NB))) return false;
  *q = (int)t;
  return true;
}

// floor(a / b) for b > 0
GM_HD int gm_floor_div(int a, int b) {
  const int q = a / b;
  return a - q * b < 0 ? q - 1 : q;
}

// the bin of the line (d_top, d_bot) at window row r of R: |d_top|, |d_bot| <= 1024 and R <= 32768 keep the numerator below 2^27
GM_HD int gm_line_bin(int d_top, int d_bot, int r, int R) {
  return gm_floor_div(2 * (d_top * (R - 1 - r) + d_bot * r) + (R - 1), 2 * (R - 1));
}

// vote << 32 | ~index: the unsigned maximum is the largest vote, then the smallest d_bot, then the smallest d_top
GM_HD unsigned long long gm_hough_key(int vote, int d_top, int d_bot, int NB) {
  return (unsigned long long)(unsigned)vote << 32 | (unsigned)~(unsigned)(d_bot * 2 * NB + d_top + NB);
}
GM_HD void gm_hough_unkey(unsigned long long key, int NB, int* vote, int* d_top, int* d_bot) {
  const unsigned idx = ~(unsigned)key;
  *vote = (int)(key >> 32);
  *d_bot = (int)(idx / (unsigned)(2 * NB));
  *d_top = (int)(idx % (unsigned)(2 * NB)) - NB;
}

// the Hough line's disparity at window row r (round 0 of the refinement)
GM_HD float gm_line_disp(int d_top, int d_bot, int r, int R) {
  return ((float)d_top * (float)(R - 1 - r) + (float)d_bot * (float)r) / (float)(R - 1);
}

// the plane's disparity at the centred coordinates (u', v')
GM_HD float gm_plane_disp(float a, float b, float c, int u, int v) { return (a * (float)u + b * (float)v) + c; }

// the Hough line as a plane in centred coordinates: a = 0, b, c
GM_HD void gm_line_plane(int d_top, int d_bot, int rows, double* b, double* c) {
  *b = (double)(d_bot - d_top) / (double)(rows - 1);
  *c = (double)d_top + *b * (double)(rows / 2);
}

// least squares over the ten sums: abc_rms = { a, b, c, rms } in pixels; false: not det > 0, and the numbers written are to be
// dropped (they are the formulas with det replaced by 1: finite, never used).  Straight-line code on purpose: the caller
// selects, nothing branches on det.
GM_HD bool gm_solve(const long long* S, double* abc_rms) {
  const double n = (double)S[GM_N], Su = (double)S[GM_SU], Sv = (double)S[GM_SV], Sq = (double)S[GM_SQ];
  const double Suu = (double)S[GM_SUU], Suv = (double)S[GM_SUV], Svv = (double)S[GM_SVV];
  const double Suq = (double)S[GM_SUQ], Svq = (double)S[GM_SVQ], Sqq = (double)S[GM_SQQ];
  const double c00 = Svv * n - Sv * Sv, c01 = Suv * n - Sv * Su, c02 = Suv * Sv - Svv * Su;
  const double c11 = Suu * n - Su * Su, c12 = Suu * Sv - Suv * Su, c22 = Suu * Svv - Suv * Suv;
  const double det = (Suu * c00 - Suv * c01) + Su * c02;
  const bool ok = det > 0.0;
  const double dd = ok ? det : 1.0;
  const double A = ((Suq * c00 - Svq * c01) + Sq * c02) / dd;
  const double B = ((Svq * c11 - Suq * c01) - Sq * c12) / dd;
  const double C = ((Suq * c02 - Svq * c12) + Sq * c22) / dd;
  const double rss = Sqq - ((A * Suq + B * Svq) + C * Sq);
  const double ms = rss / n;
  abc_rms[3] = sqrt(ms > 0.0 ? ms : 0.0) / 16.0;
  abc_rms[0] = A / 16.0;
  abc_rms[1] = B / 16.0;
  abc_rms[2] = C / 16.0;
  return ok;
}

// hs_n = { hs, nx, ny, nz }: the camera's height above the plane and the plane's unit normal in the camera frame
GM_HD void gm_pose(double a, double b, double c, double uc, double vc, double f, double baseline, double cx, double cy,
                   double doffs, double v0, double* hs_n) {
  const double c_img = ((c - a * uc) - b * (v0 + vc)) + doffs;
  const double nz = ((a * cx + b * cy) + c_img) / f;
  const double norm = sqrt((a * a + b * b) + nz * nz);
  if (!(norm > 0.0)) {
    hs_n[0] = hs_n[1] = hs_n[2] = hs_n[3] = 0.0;
    return;
  }
  hs_n[0] = baseline / norm;
  hs_n[1] = a / norm;
  hs_n[2] = b / norm;
  hs_n[3] = nz / norm;
}
