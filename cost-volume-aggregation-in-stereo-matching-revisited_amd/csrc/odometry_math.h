// The arithmetic of stereo visual odometry (include/dca_hip.h, dca_ego_motion), written ONCE for the
// kernels of odometry.hip and for the host check tools/odometry_math_check.cpp: the level cameras and the quantisation
// exponents, the bilinear sample in sixteenths of a pixel, the Jacobian of one pixel, its quantisation and Huber weight, the
// 29 integer sums, the 6x6 solve, the Cayley map, the composition and the formation of G.  The per-pixel part is fp32, the
// solve fp64; every operation is rounded on its own and only + - * / are used, so numpy restates it bit for bit.
#pragma once
#include <math.h>
#include <string.h>

#include "temporal_math.h"

#pragma clang fp contract(off)

#define OM_SUMS 29                 // 21 upper entries w q_i q_j (i <= j, row-major), 6 w q_i r, w r r, the count
#define OM_B 21
#define OM_RR 27
#define OM_N 28
#define OM_QBITS 17                // |q_i| <= 2^17 by the bound of |J_i|; below 2^18 with every rounding counted

// the camera of pyramid level l and the per-pixel constants of a sums launch
struct OmLevel {
  float f, cx, cy, doffs, min_disp, max_disp, min_ratio;
  float scale[6];                  // 2^e_i
  int H, W, grad_min, huber_k;
};

// level l of a camera in fp64: f / 2^l, (c + 0.5) / 2^l - 0.5, doffs / 2^l
inline void om_level_camera(double f, double cx, double cy, double doffs, int l, double* fl, double* cxl, double* cyl, double* dl) {
  const double s = ldexp(1.0, l);
  *fl = f / s, *cxl = (cx + 0.5) / s - 0.5, *cyl = (cy + 0.5) / s - 0.5, *dl = doffs / s;
}

// e_i with 510 max|Ju_i, Jv_i| 2^e_i <= 2^OM_QBITS over the H x W image: |gx|, |gy| <= 255 each
inline void om_exponents(double f, double cx, double cy, double doffs, double max_disp, int H, int W, int e[6]) {
  const double A = fmax(fabs(cx), fabs((double)(W - 1) - cx)), Bv = fmax(fabs(cy), fabs((double)(H - 1) - cy));
  const double Dn = max_disp + doffs;
  const double B[6] = {Dn, Dn, fmax(A, Bv) * Dn / f, fmax(A * Bv / f, f + Bv * Bv / f), fmax(f + A * A / f, A * Bv / f),
                       fmax(A, Bv)};
  for (int i = 0; i < 6; ++i) {
    int k = 0;
    frexp(510.0 * B[i], &k);       // 510 B = m 2^k with m in [0.5, 1)
    const int ei = OM_QBITS - k;
    e[i] = ei > 60 ? 60 : (ei < -60 ? -60 : ei);
  }
}

// the exact bilinear sample in 1/256 grey level at (x0 + fx / 16, y0 + fy / 16); the footprint x0 .. x0 + 1, y0 .. y0 + 1 is inside
TM_HD int om_bilinear16(const unsigned char* I, int W, int x0, int y0, int fx, int fy) {
  const unsigned char* p = I + (long)y0 * W + x0;
  return (16 - fy) * ((16 - fx) * (int)p[0] + fx * (int)p[1]) + fy * ((16 - fx) * (int)p[W] + fx * (int)p[W + 1]);
}

// w in 1/64: 64 inside the Huber radius k (in 1/256 grey level), else 64 k / |r| by integer division
TM_HD int om_weight(int r, int k) {
  const int ar = r < 0 ? -r : r;
  return ar <= k ? 64 : (64 * k) / ar;
}

struct OmPixel {
  int q[6];
  int r, w;
};

// Source pixel (u, v) of the previous level image, 1 <= u <= W - 2, 1 <= v <= H - 2: false if it takes no part.  g: G of the
// level (12 floats).  Every comparison is made in float before anything is converted.
TM_HD bool om_pixel(const OmLevel& L, const float* g, const unsigned char* Ip, const unsigned char* Ic, const float* D, int u,
                    int v, OmPixel* o) {
  const long at = (long)v * L.W + u;
  const float d = D[at];
  if (!(fabsf(d) < INFINITY && d >= L.min_disp && d < L.max_disp)) return false;
  const int gx = (int)Ip[at + 1] - (int)Ip[at - 1], gy = (int)Ip[at + L.W] - (int)Ip[at - L.W];
  if ((gx < 0 ? -gx : gx) + (gy < 0 ? -gy : gy) < L.grad_min) return false;
  const float fu = (float)u, fv = (float)v, den = d + L.doffs;
  const float x = tm_row(g, 0, fu, fv, den), y = tm_row(g, 1, fu, fv, den), z = tm_row(g, 2, fu, fv, den);
  if (!(z >= L.min_ratio)) return false;
  const float px = floorf((x / z) * 16.f + 0.5f), py = floorf((y / z) * 16.f + 0.5f);
  if (!(px >= 0.f && px < (float)((L.W - 1) * 16) && py >= 0.f && py < (float)((L.H - 1) * 16))) return false;
  const int ix = (int)px, iy = (int)py;
  o->r = om_bilinear16(Ic, L.W, ix >> 4, iy >> 4, ix & 15, iy & 15) - ((int)Ip[at] << 8);
  const float a = fu - L.cx, b = fv - L.cy, af = a / L.f, bf = b / L.f, fgx = (float)gx, fgy = (float)gy;
  float J[6];
  J[0] = fgx * den;
  J[1] = fgy * den;
  J[2] = fgx * (-(af * den)) + fgy * (-(bf * den));
  J[3] = fgx * (-(af * b)) + fgy * (-(L.f + bf * b));
  J[4] = fgx * (L.f + af * a) + fgy * (af * b);
  J[5] = fgx * (-b) + fgy * a;
#pragma unroll
  for (int i = 0; i < 6; ++i) o->q[i] = (int)rintf(J[i] * L.scale[i]);
  o->w = om_weight(o->r, L.huber_k);
  return true;
}

TM_HD void om_accumulate(long long* S, const OmPixel& p) {
  const long long w = p.w, r = p.r;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const long long wq = w * p.q[i];
#pragma unroll
    for (int j = i; j < 6; ++j) S[k++] += wq * p.q[j];
    S[OM_B + i] += wq * r;
  }
  S[OM_RR] += w * r * r;
  S[OM_N] += 1;
}

TM_HD int om_upper(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }   // index of (i, j), i <= j, among the 21

// A x = c by LDL^T in ONE written order; false if a pivot is not positive (NaN included)
TM_HD bool om_ldl_solve(const double A[6][6], const double c[6], double x[6]) {
  double L[6][6], Dg[6], y[6];
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * Dg[k];
    if (!(d > 0.0)) return false;
    Dg[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * Dg[k];
      L[i][j] = s / d;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = c[i];
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / Dg[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s;
  }
  return true;
}

// the sums of one iteration -> xi = (tau, omega): A_ij = S_ij 2^(-e_i - e_j), the diagonal times 1 + 2^-10,
// c_i = S_ir 2^(-e_i - 7)  (2^-8 for r's unit and the 2 of the central difference; w's 1/64 cancels)
TM_HD bool om_step(const long long* S, const int* e, double xi[6]) {
  double A[6][6], c[6];
  for (int i = 0; i < 6; ++i) {
    for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = (double)S[om_upper(i, j)] * ldexp(1.0, -e[i] - e[j]);
    A[i][i] = A[i][i] * (1.0 + 0.0009765625);
    c[i] = (double)S[OM_B + i] * ldexp(1.0, -e[i] - 7);
  }
  return om_ldl_solve(A, c, xi);
}

// R(omega) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = omega / 2: orthogonal in real arithmetic, I + [omega]x to first order
TM_HD void om_cayley(const double* w, double* R) {
  const double a0 = w[0] * 0.5, a1 = w[1] * 0.5, a2 = w[2] * 0.5;
  const double n = (a0 * a0 + a1 * a1) + a2 * a2, den = 1.0 + n, m = 1.0 - n;
  R[0] = (m + 2.0 * (a0 * a0)) / den, R[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den, R[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  R[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den, R[4] = (m + 2.0 * (a1 * a1)) / den, R[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  R[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den, R[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den, R[8] = (m + 2.0 * (a2 * a2)) / den;
}

// T <- T [Rw | tw]^-1 with the inverse rotation taken as the transpose: R <- R Rw^T, tau <- tau - R_new tw
TM_HD void om_compose(double* R, double* tau, const double* Rw, const double* tw) {
  double Rn[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (R[3 * i] * Rw[3 * j] + R[3 * i + 1] * Rw[3 * j + 1]) + R[3 * i + 2] * Rw[3 * j + 2];
  for (int i = 0; i < 3; ++i) {
    tau[i] = tau[i] - ((Rn[3 * i] * tw[0] + Rn[3 * i + 1] * tw[1]) + Rn[3 * i + 2] * tw[2]);
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rn[3 * i + j];
  }
}

TM_HD double om_dot3(const double* a, int sa, const double* b, int sb) { return (a[0] * b[0] + a[sa] * b[sb]) + a[2 * sa] * b[2 * sb]; }

// G = (1/f) [ K R A | K tau ] in temporal.reproject_matrix's written order (tau is already in baselines); exactly [I | 0] for
// the identity; rounded to fp32 once
TM_HD void om_form_g(const double* R, const double* tau, double f, double cx, double cy, float* g) {
  const double K[9] = {f, 0.0, cx, 0.0, f, cy, 0.0, 0.0, 1.0}, A[9] = {1.0, 0.0, -cx, 0.0, 1.0, -cy, 0.0, 0.0, f};
  double RA[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) RA[3 * i + j] = om_dot3(R + 3 * i, 1, A + j, 3);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) g[4 * i + j] = (float)(om_dot3(K + 3 * i, 1, RA + j, 3) / f);
    g[4 * i + 3] = (float)(om_dot3(K + 3 * i, 1, tau, 1) / f);
  }
}

// One Gauss-Newton update from the sums of an iteration: false (nothing changed) with fewer than min_pixels pixels or a pivot
// that is not positive
TM_HD bool om_update(const long long* S, const int* e, int min_pixels, double* R, double* tau) {
  double xi[6], Rw[9];
  if (S[OM_N] < min_pixels || !om_step(S, e, xi)) return false;
  om_cayley(xi + 3, Rw);
  om_compose(R, tau, Rw, xi);
  return true;
}

// the mean of w r^2 with w in (0, 1], in grey levels squared
TM_HD double om_residual(const long long* S) {
  return S[OM_N] > 0 ? ((double)S[OM_RR] * ldexp(1.0, -22)) / (double)S[OM_N] : 0.0;
}

// The world pose chained by one motion: W <- W T^-1 with T = (R | t) the (3,4) pose of the previous camera in the current one
// (metres) and its inverse (R^T | -R^T t); W, T row-major (3,4); in ONE written order
TM_HD void om_chain(double* W, const double* T) {
  double Ri[9], ti[3], Wn[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Ri[3 * i + j] = T[4 * j + i];
    ti[i] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Wn[4 * i + j] = (W[4 * i] * Ri[j] + W[4 * i + 1] * Ri[3 + j]) + W[4 * i + 2] * Ri[6 + j];
    Wn[4 * i + 3] = ((W[4 * i] * ti[0] + W[4 * i + 1] * ti[1]) + W[4 * i + 2] * ti[2]) + W[4 * i + 3];
  }
  for (int i = 0; i < 12; ++i) W[i] = Wn[i];
}
