// High-resolution pairs: the integer-factor area downscale of the uint8 pair and of a ground-truth
// disparity in front of the network (the reference's myImageFloder_middlebury_additional, dataloader/datasets.py:547-673),
// and joint bilateral upsampling of the network's disparity under the full-resolution left image behind it (Kopf et al.
// 2007; nothing in the reference computes it).  The definitions of include/dca_hip.h (dca_area_downscale_u8,
// dca_area_downscale_f32, dca_guided_upsample) as they are written.
//
// The downscales: one thread per output pixel, every source byte read once.
//
// The upsampler: one workgroup per HR_TH x HR_TW tile of output pixels.  Staged in LDS: the low-resolution pixels under the
// tile with a halo of r -- the disparity with the tap's validity folded in (+0.0: not a tap) and the guide colour packed
// into one word -- and the two tables.  A thread owns HR_RUN consecutive columns of one row: their low-resolution columns
// are i0 and, for s < 4, i0 + 1, so one row of taps is 2r + 2 LDS pixels read ONCE for the run, and every pixel picks its
// 2r + 1 of them.  Per pixel the taps are still added in the order a (outer), b (inner): the result does not depend on the
// run.  |dR| + |dG| + |dB| is one v_sad_u8 on the packed words.  The full-resolution guide is read once, the outputs are
// written once, as 16-byte (12-byte for three channels) accesses where the storage is aligned for them.
#include <math.h>

#include "dca_common.h"
#include "../../include/dca_hip.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define HR_THREADS DCA_HR_THREADS
#define HR_TH DCA_HR_TILE_H
#define HR_TW DCA_HR_TILE_W
#define HR_RUN DCA_HR_RUN
#define HR_RUNS_X (HR_TW / HR_RUN)                             // threads along a tile row
static_assert(HR_RUN == 4, "a run is one 16-byte store");
static_assert(HR_TW % HR_RUN == 0 && HR_RUNS_X * HR_TH == HR_THREADS, "one run per thread covers the tile");
static_assert(DCA_HR_RANGE_LEN == 3 * 255 + 1, "one entry per sum of three byte differences");

// ONE place for the geometry of the upsampler: the launcher takes the grid from it, the kernel the tile origin and the
// extent of the low-resolution tile in LDS
template <int S, int R>
struct HrGeom {
  static constexpr int LH = (HR_TH - 1) / S + 2 + 2 * R;       // low-resolution rows / columns under a tile, with the halo:
  static constexpr int LW = (HR_TW - 1) / S + 2 + 2 * R;       // a tile origin need not be a multiple of S (S = 3)
  static constexpr int NC = (S == 4 ? 0 : 1) + 2 * R + 1;      // low-resolution columns under a run, with the halo
  // a run starts at a multiple of HR_RUN: at phase 0 where S divides HR_RUN, at any phase below S otherwise
  static constexpr bool PHASE0 = HR_RUN % S == 0;
  static_assert((PHASE0 ? HR_RUN - 1 : S - 1 + HR_RUN - 1) / S <= (S == 4 ? 0 : 1), "a run spans the columns i0 (and i0 + 1)");
};
static inline dim3 hr_grid(int H, int W) { return dim3((unsigned)cdiv(W, HR_TW), (unsigned)cdiv(H, HR_TH)); }

__device__ __forceinline__ bool hr_finite(float v) { return fabsf(v) < INFINITY; }          // false for a NaN

// ---- area downscale ---------------------------------------------------------------------------------------------------
// grid (ceil(h w / HR_THREADS), 2): blockIdx.y is the image
template <int C>
__global__ __launch_bounds__(HR_THREADS) void area_u8_kernel(const unsigned char* __restrict__ left,
                                                             const unsigned char* __restrict__ right,
                                                             unsigned char* __restrict__ out, int H, int W, int h, int w, int s) {
  const int o = blockIdx.x * HR_THREADS + threadIdx.x;
  if (o >= h * w) return;
  const unsigned char* src = blockIdx.y ? right : left;
  const int j = o / w, i = o - j * w;
  const int y1 = min(H, (j + 1) * s), x1 = min(W, (i + 1) * s);
  unsigned sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = 0;
  for (int y = j * s; y < y1; ++y) {
    const unsigned char* p = src + ((long)y * W + i * s) * C;
    for (int x = i * s; x < x1; ++x, p += C) {
      if (C == 4 && ((uintptr_t)p & 3) == 0) {
        const unsigned v = *(const unsigned*)p;
        sum[0] += v & 255u, sum[1] += (v >> 8) & 255u, sum[2] += (v >> 16) & 255u, sum[C - 1] += v >> 24;
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] += p[c];
      }
    }
  }
  const unsigned cnt = (unsigned)((y1 - j * s) * (x1 - i * s));
  unsigned char* q = out + ((long)blockIdx.y * h * w + o) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = (unsigned char)((sum[c] + cnt / 2) / cnt);
}

// grid (ceil(h w / HR_THREADS))
__global__ __launch_bounds__(HR_THREADS) void area_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                              int h, int w, int s, int inf_to_zero, int flip_rows) {
  const int o = blockIdx.x * HR_THREADS + threadIdx.x;
  if (o >= h * w) return;
  const int j = o / w, i = o - j * w;
  const int y1 = min(H, (j + 1) * s), x1 = min(W, (i + 1) * s);
  float sum = 0.f;
  bool first = true;
  for (int y = j * s; y < y1; ++y) {
    const float* p = in + (long)(flip_rows ? H - 1 - y : y) * W;
    for (int x = i * s; x < x1; ++x) {
      sum = first ? p[x] : sum + p[x];                         // starting from the first pixel: -0.0 stays -0.0
      first = false;
    }
  }
  float v = (sum / (float)((y1 - j * s) * (x1 - i * s))) / (float)s;
  if (inf_to_zero && !hr_finite(v)) v = 0.f;
  out[o] = v;
}

// ---- guided upsampling -------------------------------------------------------------------------------------------------
struct HrUp {
  const float* disp_lo;
  const float* mask_lo;                                        // indexed like disp_lo, or NULL
  const unsigned char* guide_lo;
  const unsigned char* guide_hi;
  const float* ws;
  const float* wr;
  float* out;
  float* valid;
  int Wc, y0, rows, cols, H, W;
  float mask_min;
};

// the packed colours (r | g << 8 | b << 16) of pixels x0 .. x0 + 3 of the row `row` of a W-pixel image; 0 beyond W
template <int C>
__device__ __forceinline__ void hr_load_guide4(const unsigned char* __restrict__ row, int x0, int W, unsigned g[HR_RUN]) {
  const unsigned char* p = row + (long)x0 * C;
  if (x0 + HR_RUN <= W && ((uintptr_t)p & 3) == 0) {
    const unsigned* q = (const unsigned*)p;
    if (C == 4) {
#pragma unroll
      for (int k = 0; k < HR_RUN; ++k) g[k] = q[k] & 0x00ffffffu;
    } else {                                                   // 12 bytes, four pixels: three dwords
      const unsigned a = q[0], b = q[1], c = q[2];
      g[0] = a & 0x00ffffffu;
      g[1] = (a >> 24 | b << 8) & 0x00ffffffu;
      g[2] = (b >> 16 | c << 16) & 0x00ffffffu;
      g[3] = c >> 8;
    }
  } else {
#pragma unroll
    for (int k = 0; k < HR_RUN; ++k) {
      g[k] = 0;
      if (x0 + k < W) g[k] = (unsigned)p[k * C] | (unsigned)p[k * C + 1] << 8 | (unsigned)p[k * C + 2] << 16;
    }
  }
}

// four consecutive floats of a row from column x0: one 16-byte store where all four exist and the address allows it
__device__ __forceinline__ void hr_store4(float* __restrict__ row, int x0, int W, const float v[HR_RUN]) {
  float* p = row + x0;
  if (x0 + HR_RUN <= W && ((uintptr_t)p & 15) == 0) {
    // written once, not read again here: a streaming store (which also keeps hipcc from splitting it into 12 + 4 bytes to
    // share the last column's store with the branch below)
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(q, (f32x4*)p);
  } else {
#pragma unroll
    for (int k = 0; k < HR_RUN; ++k)
      if (x0 + k < W) p[k] = v[k];
  }
}

// grid hr_grid(H, W)
template <int S, int R, int C>
__global__ __launch_bounds__(HR_THREADS) void guided_upsample_kernel(HrUp u) {
  typedef HrGeom<S, R> G;
  constexpr int K = 2 * R + 1;
  __shared__ float l_d[G::LH * G::LW];                         // the disparity of an active tap, +0.0 for every other pixel
  __shared__ unsigned l_g[G::LH * G::LW];                      // r | g << 8 | b << 16
  __shared__ float l_wr[DCA_HR_RANGE_LEN];
  __shared__ float l_ws[S * K];
  const int t = threadIdx.x;
  const int ty0 = blockIdx.y * HR_TH, tx0 = blockIdx.x * HR_TW;
  const int jb = ty0 / S - R, ib = tx0 / S - R;                // the low-resolution pixel of LDS element (0, 0)
  for (int e = t; e < G::LH * G::LW; e += HR_THREADS) {
    const int j = jb + e / G::LW, i = ib + e % G::LW;
    float d = 0.f;
    unsigned g = 0;
    if (j >= 0 && j < u.rows && i >= 0 && i < u.cols) {
      const long at = (long)(u.y0 + j) * u.Wc + i;
      const float v = u.disp_lo[at];
      if (hr_finite(v) && v > 0.f && (!u.mask_lo || u.mask_lo[at] >= u.mask_min)) d = v;
      const unsigned char* p = u.guide_lo + ((long)j * u.cols + i) * C;
      g = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
    l_d[e] = d;
    l_g[e] = g;
  }
  for (int e = t; e < DCA_HR_RANGE_LEN; e += HR_THREADS) l_wr[e] = u.wr[e];
  if (t < S * K) l_ws[t] = u.ws[t];
  __syncthreads();

  const int y = ty0 + t / HR_RUNS_X, x0 = tx0 + (t % HR_RUNS_X) * HR_RUN;
  if (y >= u.H || x0 >= u.W) return;                           // (no barrier below)
  unsigned gh[HR_RUN];
  hr_load_guide4<C>(u.guide_hi + (long)y * u.W * C, x0, u.W, gh);
  const int j = y / S, py = y - j * S, i0 = x0 / S;
  const int ph = G::PHASE0 ? 0 : x0 - i0 * S;                  // the phase of the run's first pixel
  int ip[HR_RUN];                                              // pixel k of the run lies in column i0 + ip[k]: 0 or 1
  float wx[HR_RUN][K], wy[K];
#pragma unroll
  for (int k = 0; k < HR_RUN; ++k) {
    ip[k] = (ph + k) / S;
    const int px = ph + k - ip[k] * S;
#pragma unroll
    for (int b = 0; b < K; ++b) wx[k][b] = l_ws[px * K + b];
  }
#pragma unroll
  for (int a = 0; a < K; ++a) wy[a] = l_ws[py * K + a];
  float num[HR_RUN], den[HR_RUN];
#pragma unroll
  for (int k = 0; k < HR_RUN; ++k) num[k] = den[k] = 0.f;
  const int e0 = (j - R - jb) * G::LW + (i0 - R - ib);         // LDS element of the tap a = -r, b = -r of column i0
#pragma unroll
  for (int a = 0; a < K; ++a) {
    float cd[G::NC];
    unsigned cg[G::NC];
#pragma unroll
    for (int c = 0; c < G::NC; ++c) {
      cd[c] = l_d[e0 + a * G::LW + c];
      cg[c] = l_g[e0 + a * G::LW + c];
    }
#pragma unroll
    for (int k = 0; k < HR_RUN; ++k) {
#pragma unroll
      for (int b = 0; b < K; ++b) {
        const float d = (S != 4 && ip[k]) ? cd[b + (S != 4)] : cd[b];
        const unsigned g = (S != 4 && ip[k]) ? cg[b + (S != 4)] : cg[b];
        if (d > 0.f) {
          const float wgt = (wy[a] * wx[k][b]) * l_wr[__builtin_amdgcn_sad_u8(gh[k], g, 0u)];
          num[k] = num[k] + wgt * d;
          den[k] = den[k] + wgt;
        }
      }
    }
  }
  float o[HR_RUN], v[HR_RUN];
#pragma unroll
  for (int k = 0; k < HR_RUN; ++k) {
    const bool ok = den[k] > 0.f;
    o[k] = ok ? (num[k] / den[k]) * (float)S : 0.f;
    v[k] = ok ? 1.f : 0.f;
  }
  if (u.out) hr_store4(u.out + (long)y * u.W, x0, u.W, o);
  if (u.valid) hr_store4(u.valid + (long)y * u.W, x0, u.W, v);
}

template <int S, int R>
void hr_launch(const HrUp& u, int C, hipStream_t stream) {
  const dim3 grid = hr_grid(u.H, u.W);
  if (C == 3)
    hipLaunchKernelGGL((guided_upsample_kernel<S, R, 3>), grid, dim3(HR_THREADS), 0, stream, u);
  else
    hipLaunchKernelGGL((guided_upsample_kernel<S, R, 4>), grid, dim3(HR_THREADS), 0, stream, u);
}

template <int S>
void hr_launch_r(const HrUp& u, int C, int r, hipStream_t stream) {
  if (r == 1) hr_launch<S, 1>(u, C, stream);
  else if (r == 2) hr_launch<S, 2>(u, C, stream);
  else hr_launch<S, 3>(u, C, stream);
}

inline bool hr_image_ok(int H, int W, int C, int s) {
  return H > 0 && W > 0 && (long)H * W < (1L << 31) && (C == 3 || C == 4) && s >= 2 && s <= DCA_HR_MAX_SCALE;
}

}  // namespace

extern "C" int dca_area_downscale_u8(const unsigned char* left, const unsigned char* right, unsigned char* out, int H, int W,
                                     int C, int s, hipStream_t stream) {
  DCA_REQUIRE(left && right && out && out != left && out != right && hr_image_ok(H, W, C, s));
  const int h = cdiv(H, s), w = cdiv(W, s);
  const dim3 grid((unsigned)cdiv((long)h * w, HR_THREADS), 2);
  if (C == 3)
    hipLaunchKernelGGL(area_u8_kernel<3>, grid, dim3(HR_THREADS), 0, stream, left, right, out, H, W, h, w, s);
  else
    hipLaunchKernelGGL(area_u8_kernel<4>, grid, dim3(HR_THREADS), 0, stream, left, right, out, H, W, h, w, s);
  return dca_launch_status();
}

extern "C" int dca_area_downscale_f32(const float* in, float* out, int H, int W, int s, int inf_to_zero, int flip_rows,
                                      hipStream_t stream) {
  DCA_REQUIRE(in && out && in != out && hr_image_ok(H, W, 3, s));
  DCA_REQUIRE((inf_to_zero == 0 || inf_to_zero == 1) && (flip_rows == 0 || flip_rows == 1));
  const int h = cdiv(H, s), w = cdiv(W, s);
  hipLaunchKernelGGL(area_f32_kernel, dim3((unsigned)cdiv((long)h * w, HR_THREADS)), dim3(HR_THREADS), 0, stream, in, out, H,
                     W, h, w, s, inf_to_zero, flip_rows);
  return dca_launch_status();
}

extern "C" int dca_guided_upsample(const float* disp_lo, const float* mask_lo, const unsigned char* guide_lo,
                                   const unsigned char* guide_hi, const float* ws, const float* wr, float* out, float* valid,
                                   int Hc, int Wc, int y0, int rows, int cols, int H, int W, int C, int s, int r,
                                   float mask_min, hipStream_t stream) {
  DCA_REQUIRE(disp_lo && guide_lo && guide_hi && ws && wr && (out || valid) && hr_image_ok(H, W, C, s));
  DCA_REQUIRE(r >= 1 && r <= DCA_HR_MAX_RADIUS && dca_window_ok(Hc, Wc, y0, rows, cols));
  DCA_REQUIRE(cdiv(H, s) == rows && cdiv(W, s) == cols && !(mask_lo && mask_min != mask_min));
  DCA_REQUIRE(out != disp_lo && valid != disp_lo && (!mask_lo || (out != mask_lo && valid != mask_lo)) && out != valid);
  const HrUp u = {disp_lo, mask_lo, guide_lo, guide_hi, ws, wr, out, valid, Wc, y0, rows, cols, H, W, mask_min};
  if (s == 2) hr_launch_r<2>(u, C, r, stream);
  else if (s == 3) hr_launch_r<3>(u, C, r, stream);
  else hr_launch_r<4>(u, C, r, stream);
  return dca_launch_status();
}
