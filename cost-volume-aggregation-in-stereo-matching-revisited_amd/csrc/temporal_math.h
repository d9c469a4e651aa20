// The per-pixel arithmetic of temporal stereo (include/dca_hip.h, dca_disp_reproject / dca_temporal_fuse), written ONCE for
// the kernels of temporal.hip and for the host check tools/temporal_math_check.cpp: the projection of a source pixel by the
// matrix G, its keep test and scatter key, the visibility test and the payload of a winner, and the five cases of the fusion.
// Every function is the header's formula as it is written, each operation rounded on its own.
#pragma once
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define TM_HD __host__ __device__ inline
#else
#define TM_HD inline
#endif

#pragma clang fp contract(off)

struct TmProj {
  float g[12];                     // G, row-major 3 x 4
  float doffs, min_disp, max_disp, min_ratio;
  int H, W;
};

TM_HD unsigned tm_bits(float v) {
  unsigned b;
  memcpy(&b, &v, sizeof b);
  return b;
}
TM_HD float tm_float(unsigned b) {
  float v;
  memcpy(&v, &b, sizeof v);
  return v;
}

// row r of G applied to (u, v, 1, den)
TM_HD float tm_row(const float* g, int r, float u, float v, float den) {
  return ((g[4 * r] * u + g[4 * r + 1] * v) + g[4 * r + 2]) + g[4 * r + 3] * den;
}

// z = Z_cur / Z_prev of the source pixel (u, v) with disparity d
TM_HD float tm_ratio(const TmProj& p, int u, int v, float d) { return tm_row(p.g, 2, (float)u, (float)v, d + p.doffs); }

// The source pixel (u, v) with disparity d, its mask already applied by the caller: true if it is kept, then *target = vf W + uf
// and *denp = den'.  Every comparison is made in float before anything is converted: a NaN fails, an infinity or 1e30 fails
// without overflowing an int.  d >= min_disp >= 0 and doffs >= 0 make den' >= 0, so its bits order as the floats do.
TM_HD bool tm_project(const TmProj& p, int u, int v, float d, long* target, float* denp) {
  const float fu = (float)u, fv = (float)v;
  const float den = d + p.doffs;
  const float x = tm_row(p.g, 0, fu, fv, den), y = tm_row(p.g, 1, fu, fv, den), z = tm_row(p.g, 2, fu, fv, den);
  const float up = x / z, vp = y / z;
  const float uf = floorf(up + 0.5f), vf = floorf(vp + 0.5f);
  const float dn = den / z;
  const float dp = dn - p.doffs;
  const bool keep = fabsf(d) < INFINITY && d >= p.min_disp && z >= p.min_ratio && uf >= 0.f && uf < (float)p.W && vf >= 0.f &&
                    vf < (float)p.H && dp >= p.min_disp && dp < p.max_disp;
  if (!keep) return false;
  *target = (long)(int)vf * p.W + (int)uf;
  *denp = dn;
  return true;
}

// bits(den') << 32 | (0xFFFFFFFF - source index): the unsigned maximum is the nearest surface, then the smallest source index
TM_HD unsigned long long tm_key(float denp, long src) {
  return (unsigned long long)tm_bits(denp) << 32 | (unsigned long long)(0xFFFFFFFFu - (unsigned)src);
}
TM_HD float tm_key_den(unsigned long long key) { return tm_float((unsigned)(key >> 32)); }
TM_HD long tm_key_src(unsigned long long key) { return (long)(0xFFFFFFFFu - (unsigned)key); }

// the winner of a target against the largest den' of its window: an absolute threshold in pixels
TM_HD bool tm_visible(float denp, float occl_px, float denmax) { return denp + occl_px >= denmax; }

// the payload of a visible winner, z recomputed from its source pixel
TM_HD float tm_pred_var(float var_src, float z, float q) { return var_src / (z * z) + q; }
TM_HD unsigned char tm_pred_age(unsigned char age_src) { return age_src == 255 ? 255 : (unsigned char)(age_src + 1); }

// The fusion of one pixel.  m_ok: the measurement m is finite, >= min_disp, its mask passes and its variance vm is positive and
// finite (the caller's test); p_ok = pred > 0 && 0 <= pred_var <= var_max.  innov = |m - pred| where both are valid, else +0.0.
struct TmState {
  float disp, var, innov;
  unsigned char age;
};
TM_HD bool tm_pred_ok(float pred, float pred_var, float var_max) { return pred > 0.f && pred_var >= 0.f && pred_var <= var_max; }
TM_HD bool tm_meas_ok(float m, float vm, float min_disp) {
  return fabsf(m) < INFINITY && m >= min_disp && vm > 0.f && vm < INFINITY;
}
TM_HD TmState tm_fuse(bool m_ok, float m, float vm, bool p_ok, float pred, float pred_var, unsigned char pred_age, float gate2) {
  TmState r = {0.f, 0.f, 0.f, 0};
  if (m_ok && p_ok) {
    const float e = m - pred, s = pred_var + vm;
    r.innov = fabsf(e);
    if (e * e <= gate2 * s) {
      const float k = pred_var / s;
      r.disp = pred + k * e;
      r.var = pred_var - k * pred_var;
      r.age = pred_age;
    } else {                        // a new surface: the filter starts again
      r.disp = m;
      r.var = vm;
    }
  } else if (m_ok) {
    r.disp = m;
    r.var = vm;
  } else if (p_ok) {                // coast
    r.disp = pred;
    r.var = pred_var;
    r.age = pred_age;
  }
  return r;
}
