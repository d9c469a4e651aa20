// Self-supervised stereo loss (definitions: include/dca_hip.h, dca_selfsup_loss_fwd): the right image
// warped along the row by a predicted disparity, compared with the left image (3x3 SSIM + L1 at interior pixels, masked by
// in-view x valid), plus the reference's edge-aware smoothness term (util.py:76-86 loss_disp_smoothness, which it never
// calls).  All `nlev` disparity maps of a step go through ONE launch per direction, the level being a grid dimension.
//
//  * forward  -- 64 x 16 pixel tiles with a ONE-pixel halo in LDS, channel by channel: the warped channel Y_c is
//    recomputed from the disparity tile and two gathered right-image samples (never stored in global memory), the 3x3
//    window moments are taken around the window mean (E[(I - mu)^2]: the same number as E[I^2] - mu^2 without its
//    cancellation).  Each workgroup writes its four partial sums (sum M e, sum M, sum |dd| w, sum w) as doubles into a slot
//    of its own; a second, one-workgroup launch adds them in a fixed order and leaves per level
//    (photo, smooth, sum M, 1 / max(sum M, 1), 1 / sum w) and the weighted total on the device.
//  * backward -- the same tiles with a TWO-pixel halo: the window terms are computed once per window q of the tile + 1
//    (P_q, Q_q, T_q and the two means, already scaled by the window's mask and clamp), then every pixel p collects
//    P_q + Q_q (I_p - muI_q) - T_q (Y_p - muY_q) from the nine windows that contain it, adds the L1 term, multiplies by
//    dY/dd (recomputed from the right image) and adds the smoothness term.  Every gradient element is written once.
// No atomics, no host synchronisation, plain launches on the caller's stream: bitwise reproducible and graph-capturable.
#include "dca_common.h"

namespace {

constexpr int TW = DCA_SELFSUP_TILE_W, TH = DCA_SELFSUP_TILE_H, NT = 256;
constexpr int LMAX = DCA_SELFSUP_MAX_LEVELS, NSUM = DCA_SELFSUP_SUMS, NOUT = DCA_SELFSUP_OUT;
constexpr int ROWS = NT / TW;               // tile rows one pass of the workgroup covers
constexpr int PPT = TH / ROWS;              // pixels per thread: rows ly0 + k ROWS, one column
constexpr int P1W = TW + 2, NP1 = (TH + 2) * P1W;       // tile + 1
constexpr int P2W = TW + 4, NP2 = (TH + 4) * P2W;       // tile + 2
static_assert(NT % TW == 0 && TH % ROWS == 0 && NT / 64 == 4, "thread <-> pixel mapping, four waves");

struct SsArgs {
  const float* d[LMAX];
  float* g[LMAX];
  float w[LMAX];
  int nlev;
};

// the warp of one pixel: Y = R[x0] + t (R[x0 + 1] - R[x0]); 0 <= x0 <= W - 2 for ANY d (fmaxf / fminf drop a NaN)
struct Warp {
  int x0;
  float t;
  bool inview, moves;                       // moves: 0 < xs < W - 1, the only place where dY/dd != 0
};
__device__ __forceinline__ Warp warp_of(float d, int x, int W) {
  const float xs = (float)x - d, hi = (float)(W - 1);
  const float xc = fminf(fmaxf(xs, 0.f), hi);
  int x0 = (int)floorf(xc);
  x0 = x0 < W - 2 ? x0 : W - 2;
  return {x0, xc - (float)x0, xs >= 0.f && xs <= hi, xs > 0.f && xs < hi};
}

__device__ __forceinline__ float valid_at(const void* v, int u8, long i) {
  if (!v) return 1.f;
  return u8 ? (float)((const unsigned char*)v)[i] : ((const float*)v)[i];
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// 3x3 window around LDS index `ctr` of two planes of row pitch `pitch`
struct Win {
  float mi, my, N1, N2, D1, D2, S;
};
__device__ __forceinline__ Win window(const float* sI, const float* sY, int ctr, int pitch, float c1, float c2) {
  float si = 0.f, sy = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      si += sI[ctr + dy * pitch + dx];
      sy += sY[ctr + dy * pitch + dx];
    }
  Win w;
  w.mi = si * (1.f / 9.f);
  w.my = sy * (1.f / 9.f);
  float vi = 0.f, vy = 0.f, cv = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float p = sI[ctr + dy * pitch + dx] - w.mi, q = sY[ctr + dy * pitch + dx] - w.my;
      vi += p * p;
      vy += q * q;
      cv += p * q;
    }
  w.N1 = 2.f * w.mi * w.my + c1;
  w.N2 = 2.f * (cv * (1.f / 9.f)) + c2;
  w.D1 = w.mi * w.mi + w.my * w.my + c1;
  w.D2 = (vi + vy) * (1.f / 9.f) + c2;
  w.S = (w.N1 * w.N2) / (w.D1 * w.D2);
  return w;
}

// one channel of the left image and of the warped right image for the tile + HALO (zeros outside the image)
template <int HALO>
__device__ __forceinline__ void stage_channel(float* sI, float* sY, const float* sD, const float* Ic, const float* Rc, int ty0,
                                              int tx0, int H, int W, bool warp) {
  constexpr int PW = TW + 2 * HALO, NP = (TH + 2 * HALO) * PW;
  for (int i = threadIdx.x; i < NP; i += NT) {
    const int gy = ty0 - HALO + i / PW, gx = tx0 - HALO + i % PW;
    float iv = 0.f, yv = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      iv = Ic[gy * W + gx];
      if (warp) {
        const Warp w = warp_of(sD[i], gx, W);
        const float r0 = Rc[gy * W + w.x0], r1 = Rc[gy * W + w.x0 + 1];
        yv = r0 + w.t * (r1 - r0);
      }
    }
    sI[i] = iv;
    sY[i] = yv;
  }
}

template <int HALO>
__device__ __forceinline__ void stage_disp(float* sD, const float* d, int ty0, int tx0, int H, int W) {
  constexpr int PW = TW + 2 * HALO, NP = (TH + 2 * HALO) * PW;
  for (int i = threadIdx.x; i < NP; i += NT) {
    const int gy = ty0 - HALO + i / PW, gx = tx0 - HALO + i % PW;
    sD[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? d[gy * W + gx] : 0.f;
  }
}

// part[((lev B + b) tiles + tile) NSUM + j]: sum M e, sum M, sum |dd| w, sum w over the tile's pixels
__global__ __launch_bounds__(NT) void selfsup_fwd_kernel(SsArgs a, const float* __restrict__ I, const float* __restrict__ R,
                                                         const void* __restrict__ valid, int valid_u8,
                                                         double* __restrict__ part, int H, int W, int tiles_x, float alpha,
                                                         float c1, float c2, int photo_on) {
  __shared__ float sD[NP1], sI[NP1], sY[NP1];
  __shared__ double red[NSUM][NT / 64];
  const int lev = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int HW = H * W;                                       // 3 H W < 2^31
  const float* Ib = I + (long)b * 3 * HW;
  const float* Rb = R + (long)b * 3 * HW;
  const int lx = tid % TW, ly0 = tid / TW, gx = tx0 + lx;
  float ssim[PPT], l1[PPT], ax[PPT], ay[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) ssim[k] = l1[k] = ax[k] = ay[k] = 0.f;

  stage_disp<1>(sD, a.d[lev] + (long)b * HW, ty0, tx0, H, W);
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                          // sD is complete; the previous channel has been read
    stage_channel<1>(sI, sY, sD, Ib + c * HW, Rb + c * HW, ty0, tx0, H, W, photo_on != 0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int ly = ly0 + k * ROWS, gy = ty0 + ly, ctr = (ly + 1) * P1W + lx + 1;
      if (gy < H && gx < W) {
        const float ic = sI[ctr];
        if (gx + 1 < W) ax[k] += fabsf(ic - sI[ctr + 1]);
        if (gy + 1 < H) ay[k] += fabsf(ic - sI[ctr + P1W]);
        if (photo_on && gy >= 1 && gy <= H - 2 && gx >= 1 && gx <= W - 2) {
          const Win w = window(sI, sY, ctr, P1W, c1, c2);
          ssim[k] += fminf(fmaxf((1.f - w.S) * 0.5f, 0.f), 1.f);
          l1[k] += fabsf(ic - sY[ctr]);
        }
      }
    }
  }

  double s[NSUM] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int ly = ly0 + k * ROWS, gy = ty0 + ly, ctr = (ly + 1) * P1W + lx + 1;
    if (gy < H && gx < W) {
      const float dc = sD[ctr];
      if (gx + 1 < W) {
        const float wx = expf(-ax[k] * (1.f / 3.f));
        s[2] += (double)(fabsf(dc - sD[ctr + 1]) * wx);
        s[3] += (double)wx;
      }
      if (gy + 1 < H) {
        const float wy = expf(-ay[k] * (1.f / 3.f));
        s[2] += (double)(fabsf(dc - sD[ctr + P1W]) * wy);
        s[3] += (double)wy;
      }
      if (photo_on && gy >= 1 && gy <= H - 2 && gx >= 1 && gx <= W - 2) {
        const float m = warp_of(dc, gx, W).inview ? valid_at(valid, valid_u8, (long)b * HW + gy * W + gx) : 0.f;
        const float e = alpha * (ssim[k] * (1.f / 3.f)) + (1.f - alpha) * (l1[k] * (1.f / 3.f));
        s[0] += (double)(m * e);
        s[1] += (double)m;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NSUM; ++j) {
    s[j] = wave_sum_d(s[j]);
    if ((tid & 63) == 0) red[j][tid >> 6] = s[j];
  }
  __syncthreads();
  if (tid < NSUM)
    part[(((long)lev * gridDim.y + b) * gridDim.x + blockIdx.x) * NSUM + tid] =
        ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// out[lev NOUT + ...] = photo, smooth, sum M, 1 / max(sum M, 1), 1 / sum w;  out[nlev NOUT] = sum_l w_l (ps photo + lam smooth)
__global__ __launch_bounds__(NT) void selfsup_finalize_kernel(SsArgs a, const double* __restrict__ part, int per_level,
                                                              float lam, float photo_scale, float* __restrict__ out) {
  __shared__ double red[NSUM][NT / 64];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int lev = 0; lev < a.nlev; ++lev) {
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < per_level; i += NT)
#pragma unroll
      for (int j = 0; j < NSUM; ++j) s[j] += part[((long)lev * per_level + i) * NSUM + j];
    __syncthreads();                                          // the previous level's sums have been read
#pragma unroll
    for (int j = 0; j < NSUM; ++j) {
      s[j] = wave_sum_d(s[j]);
      if ((tid & 63) == 0) red[j][tid >> 6] = s[j];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int j = 0; j < NSUM; ++j) s[j] = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
      const double inv_m = 1.0 / (s[1] > 1.0 ? s[1] : 1.0), inv_w = s[3] > 0.0 ? 1.0 / s[3] : 0.0;
      const double photo = s[0] * inv_m, smooth = s[2] * inv_w;
      float* o = out + lev * NOUT;
      o[0] = (float)photo;
      o[1] = (float)smooth;
      o[2] = (float)s[1];
      o[3] = (float)inv_m;
      o[4] = (float)inv_w;
      total += (double)a.w[lev] * ((double)photo_scale * photo + (double)lam * smooth);
    }
  }
  if (tid == 0) out[a.nlev * NOUT] = (float)total;
}

// g[lev][b, p] = gloss w_lev (ps / max(sum M, 1) dphoto/dd + lam / sum w dsmooth/dd)
__global__ __launch_bounds__(NT) void selfsup_bwd_kernel(SsArgs a, const float* __restrict__ I, const float* __restrict__ R,
                                                         const void* __restrict__ valid, int valid_u8,
                                                         const float* __restrict__ out, const float* __restrict__ gloss,
                                                         int H, int W, int tiles_x, float alpha, float lam, float c1,
                                                         float c2, float photo_scale) {
  __shared__ float sD[NP2], sI[NP2], sY[NP2];                 // tile + 2
  __shared__ float sM[NP1], sP[NP1], sQ[NP1], sT[NP1], sMI[NP1], sMY[NP1];   // per window of the tile + 1
  const int lev = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int HW = H * W;
  const float* Ib = I + (long)b * 3 * HW;
  const float* Rb = R + (long)b * 3 * HW;
  const int lx = tid % TW, ly0 = tid / TW, gx = tx0 + lx;
  const bool photo_on = photo_scale != 0.f;
  float gph[PPT], ax0[PPT], ax1[PPT], ay0[PPT], ay1[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) gph[k] = ax0[k] = ax1[k] = ay0[k] = ay1[k] = 0.f;

  stage_disp<2>(sD, a.d[lev] + (long)b * HW, ty0, tx0, H, W);
  __syncthreads();
  // the mask of every window centre q of the tile + 1: in-view x valid at interior pixels of the image, 0 elsewhere
  for (int j = tid; j < NP1; j += NT) {
    const int qy = ty0 - 1 + j / P1W, qx = tx0 - 1 + j % P1W;
    float m = 0.f;
    if (photo_on && qy >= 1 && qy <= H - 2 && qx >= 1 && qx <= W - 2) {
      const float dq = sD[(j / P1W + 1) * P2W + j % P1W + 1];
      m = warp_of(dq, qx, W).inview ? valid_at(valid, valid_u8, (long)b * HW + qy * W + qx) : 0.f;
    }
    sM[j] = m;
  }
  const float ks = -0.5f * alpha * (1.f / 3.f) * (1.f / 9.f);   // d e / d SSIM_c inside the clamp, and the window's 1/9
  const float kl = (1.f - alpha) * (1.f / 3.f);
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                          // sM is complete; the previous channel has been read
    stage_channel<2>(sI, sY, sD, Ib + c * HW, Rb + c * HW, ty0, tx0, H, W, photo_on);
    __syncthreads();
    if (photo_on) {
      for (int j = tid; j < NP1; j += NT) {
        const float m = sM[j];
        float P = 0.f, Q = 0.f, T = 0.f, mi = 0.f, my = 0.f;
        if (m != 0.f && alpha != 0.f) {
          const Win w = window(sI, sY, (j / P1W + 1) * P2W + j % P1W + 1, P2W, c1, c2);
          const float h = (1.f - w.S) * 0.5f;
          const float k = (h > 0.f && h < 1.f) ? m * ks : 0.f;
          const float idd = 1.f / (w.D1 * w.D2);
          P = k * (2.f * w.mi * w.N2 * idd - 2.f * w.my * w.S / w.D1);
          Q = k * (2.f * w.N1 * idd);
          T = k * (2.f * w.S / w.D2);
          mi = w.mi;
          my = w.my;
        }
        sP[j] = P, sQ[j] = Q, sT[j] = T, sMI[j] = mi, sMY[j] = my;
      }
      __syncthreads();
    }
#pragma unroll 1                                             // 72 registers instead of 213: three workgroups per CU
    for (int k = 0; k < PPT; ++k) {
      const int ly = ly0 + k * ROWS, gy = ty0 + ly;
      if (gy < H && gx < W) {
        const int c2i = (ly + 2) * P2W + lx + 2, c1i = (ly + 1) * P1W + lx + 1;
        const float ip = sI[c2i];
        if (gx + 1 < W) ax0[k] += fabsf(ip - sI[c2i + 1]);
        if (gx >= 1) ax1[k] += fabsf(sI[c2i - 1] - ip);
        if (gy + 1 < H) ay0[k] += fabsf(ip - sI[c2i + P2W]);
        if (gy >= 1) ay1[k] += fabsf(sI[c2i - P2W] - ip);
        if (photo_on) {
          const Warp w = warp_of(sD[c2i], gx, W);
          if (w.moves) {                                      // otherwise dY/dd = 0
            const float yp = sY[c2i];
            float acc = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
              for (int dx = -1; dx <= 1; ++dx) {
                const int j = c1i + dy * P1W + dx;
                acc += sP[j] + sQ[j] * (ip - sMI[j]) - sT[j] * (yp - sMY[j]);
              }
            acc += sM[c1i] * kl * sgn(yp - ip);               // sM = 0 off the interior
            const float* r = Rb + c * HW + gy * W + w.x0;
            gph[k] += acc * -(r[1] - r[0]);
          }
        }
      }
    }
  }

  const float* o = out + lev * NOUT;
  const float gw = gloss[0] * a.w[lev], kp = photo_scale * o[3], ksm = lam * o[4];
  float* g = a.g[lev] + (long)b * HW;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int ly = ly0 + k * ROWS, gy = ty0 + ly;
    if (gy < H && gx < W) {
      const int c2i = (ly + 2) * P2W + lx + 2;
      const float dc = sD[c2i];
      float gs = 0.f;
      if (gx + 1 < W) gs += sgn(dc - sD[c2i + 1]) * expf(-ax0[k] * (1.f / 3.f));
      if (gx >= 1) gs -= sgn(sD[c2i - 1] - dc) * expf(-ax1[k] * (1.f / 3.f));
      if (gy + 1 < H) gs += sgn(dc - sD[c2i + P2W]) * expf(-ay0[k] * (1.f / 3.f));
      if (gy >= 1) gs -= sgn(sD[c2i - P2W] - dc) * expf(-ay1[k] * (1.f / 3.f));
      g[gy * W + gx] = gw * (kp * gph[k] + ksm * gs);
    }
  }
}

struct SsGeom {
  int tiles_x, tiles;
};
int selfsup_setup(SsArgs& a, SsGeom& geo, const float* const* disps, float* const* gdisps, const float* weights, int nlev,
                  int B, int H, int W) {
  if (!disps || !weights || nlev < 1 || nlev > LMAX) return 0;
  if (B < 1 || B > 65535 || H < 3 || W < 3 || W > (1 << 24) || 3L * H * W >= (1L << 31)) return 0;
  a.nlev = nlev;
  for (int i = 0; i < LMAX; ++i) {
    a.d[i] = i < nlev ? disps[i] : nullptr;
    a.g[i] = (gdisps && i < nlev) ? gdisps[i] : nullptr;
    a.w[i] = i < nlev ? weights[i] : 0.f;
    if (i < nlev && (!a.d[i] || (gdisps && (!a.g[i] || a.g[i] == a.d[i])))) return 0;
  }
  geo.tiles_x = cdiv(W, TW);
  geo.tiles = geo.tiles_x * cdiv(H, TH);
  return 1;
}

}  // namespace

extern "C" int dca_selfsup_loss_fwd(const float* left, const float* right, const float* const* disps, const float* weights,
                                    int nlev, const void* valid, int valid_u8, double* work, float* out, int B, int H, int W,
                                    float alpha, float lam, float c1, float c2, float photo_scale, hipStream_t stream) {
  SsArgs a;
  SsGeom geo;
  DCA_REQUIRE(selfsup_setup(a, geo, disps, nullptr, weights, nlev, B, H, W));
  DCA_REQUIRE(left && right && work && out && (valid_u8 == 0 || valid_u8 == 1));
  DCA_REQUIRE(alpha >= 0.f && alpha <= 1.f && c1 > 0.f && c2 > 0.f && lam == lam && photo_scale == photo_scale);
  hipLaunchKernelGGL(selfsup_fwd_kernel, dim3(geo.tiles, B, nlev), dim3(NT), 0, stream, a, left, right, valid, valid_u8, work,
                     H, W, geo.tiles_x, alpha, c1, c2, photo_scale != 0.f ? 1 : 0);
  hipLaunchKernelGGL(selfsup_finalize_kernel, dim3(1), dim3(NT), 0, stream, a, work, B * geo.tiles, lam, photo_scale, out);
  return dca_launch_status();
}

extern "C" int dca_selfsup_loss_bwd(const float* left, const float* right, const float* const* disps, float* const* gdisps,
                                    const float* weights, int nlev, const void* valid, int valid_u8, const float* out,
                                    const float* gloss, int B, int H, int W, float alpha, float lam, float c1, float c2,
                                    float photo_scale, hipStream_t stream) {
  SsArgs a;
  SsGeom geo;
  DCA_REQUIRE(gdisps && selfsup_setup(a, geo, disps, gdisps, weights, nlev, B, H, W));
  DCA_REQUIRE(left && right && out && gloss && (valid_u8 == 0 || valid_u8 == 1));
  DCA_REQUIRE(alpha >= 0.f && alpha <= 1.f && c1 > 0.f && c2 > 0.f && lam == lam && photo_scale == photo_scale);
  hipLaunchKernelGGL(selfsup_bwd_kernel, dim3(geo.tiles, B, nlev), dim3(NT), 0, stream, a, left, right, valid, valid_u8, out,
                     gloss, H, W, geo.tiles_x, alpha, lam, c1, c2, photo_scale);
  return dca_launch_status();
}
