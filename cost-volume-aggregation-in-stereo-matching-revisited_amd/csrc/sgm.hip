// Semi-global matching on a census cost (nothing in the reference computes it): the definition of
// include/dca_hip.h (dca_sgm_disparity) as it is written, the arithmetic itself in sgm_math.h, which the host check
// tools/sgm_math_check.cpp compiles too.
//
// The launches, the kernel boundary being the only global synchronisation:
//  1. census: one thread per pixel, both images in one grid (z); a 32 x 8 tile of grey values with its 4 x 3 halo in LDS, the
//             halo outside the image filled with 255, which is below no centre.
//  2. paths:  one launch per direction, one WAVE per scanline: a row for the horizontal paths; for the others a start column, the
//             column moving by dx per row and re-entering on the other side, where a new path starts (its predecessor lies
//             outside the image) -- so every direction has exactly W equally long scanlines and every pixel lies on one.  Lane l
//             holds the KB = ceil(D / 64) consecutive bins l KB .. l KB + KB - 1 of L_r in registers: only the two edge bins need
//             a neighbour lane, and m is a cross-lane minimum.  The cost is popcount(cL ^ cR) of the census words, never stored.
//             The census words and the old S of step t + 1 are fetched before step t is computed, so the dependent chain of a
//             scan is the recursion alone.  The first direction writes S, the others add to it: integer sums, each pixel touched
//             by one wave per launch, the launches ordered by the stream.
//  3. winner-take-all: one wave per pixel, lanes over the bins (coalesced), keys S << 9 | d reduced by cross-lane minima.
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "sgm_math.h"

namespace {

static_assert(DCA_SGM_MAX_P == SGM_MAX_P && DCA_SGM_COST_OUT == SGM_COST_OUT, "sgm_math.h states the bounds for these values");
static_assert(DCA_SGM_MAX_DISP <= 4 * DCA_WAVE, "a lane holds at most four bins");
static_assert(DCA_SGM_MAX_DISP <= 512, "the key keeps d in 9 bits");
static_assert(8 * (DCA_SGM_COST_OUT + DCA_SGM_MAX_P) < 65536, "S fits uint16");

#define SGM_TILE_W 32
#define SGM_TILE_H 8
#define SGM_HALO_X 4
#define SGM_HALO_Y 3
#define SGM_LDS_W (SGM_TILE_W + 2 * SGM_HALO_X)
#define SGM_LDS_H (SGM_TILE_H + 2 * SGM_HALO_Y)
#define SGM_WTA_THREADS 256

typedef unsigned long long u64;

// ---- 1. census: grid (ceil(W / 32), ceil(H / 8), 2) -------------------------------------------------------------------------
__global__ __launch_bounds__(SGM_TILE_W* SGM_TILE_H) void sgm_census_kernel(const unsigned char* __restrict__ left,
                                                                            const unsigned char* __restrict__ right,
                                                                            u64* __restrict__ census, int H, int W, int C) {
  __shared__ unsigned char g[SGM_LDS_H][SGM_LDS_W];
  const unsigned char* img = blockIdx.z ? right : left;
  const int x0 = blockIdx.x * SGM_TILE_W, y0 = blockIdx.y * SGM_TILE_H;
  for (int i = threadIdx.x; i < SGM_LDS_H * SGM_LDS_W; i += SGM_TILE_W * SGM_TILE_H) {
    const int ly = i / SGM_LDS_W, lx = i - ly * SGM_LDS_W, y = y0 + ly - SGM_HALO_Y, x = x0 + lx - SGM_HALO_X;
    int v = 255;                                             // outside the image: below no centre
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const unsigned char* p = img + ((long)y * W + x) * C;
      v = C == 1 ? (int)p[0] : sgm_grey(p[0], p[1], p[2]);
    }
    g[ly][lx] = (unsigned char)v;
  }
  __syncthreads();
  const int tx = threadIdx.x % SGM_TILE_W, ty = threadIdx.x / SGM_TILE_W, x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const int c = g[ty + SGM_HALO_Y][tx + SGM_HALO_X];
  u64 bits = 0;
#pragma unroll
  for (int dy = 0; dy <= 2 * SGM_HALO_Y; ++dy) {
#pragma unroll
    for (int dx = 0; dx <= 2 * SGM_HALO_X; ++dx) {
      if (dy == SGM_HALO_Y && dx == SGM_HALO_X) continue;
      bits = bits << 1 | (u64)((int)g[ty + dy][tx + dx] < c ? 1 : 0);
    }
  }
  census[((long)blockIdx.z * H + y) * W + x] = bits;
}

// ---- 2. one direction of the aggregation: grid (dy == 0 ? H : W), one wave -------------------------------------------------------
struct SgmScan {
  int H, W, D, P1, P2, dy, dx, first;
};

__device__ __forceinline__ int sgm_wave_min(int v) {
#pragma unroll
  for (int o = DCA_WAVE / 2; o > 0; o >>= 1) v = sgm_min(v, __shfl_xor(v, o, DCA_WAVE));
  return v;
}

template <int KB>
struct SgmFetch {
  u64 cl, cr[KB];
  unsigned short old[KB];
};

// what a step at (y, x) reads.  Every address is clamped into the image (the row, the bins), so that no load is predicated; a
// clamped value is never used: the cost of x - d < 0 is the constant and a bin d >= D is SGM_NONE.
template <int KB>
__device__ __forceinline__ void sgm_fetch(const u64* __restrict__ cL, const u64* __restrict__ cR, const unsigned short* S,
                                          const SgmScan& a, int y, int x, int d0, SgmFetch<KB>& f) {
  const long p = (long)y * a.W + x;
  f.cl = cL[p];
#pragma unroll
  for (int j = 0; j < KB; ++j) f.cr[j] = cR[p - sgm_min(d0 + j, x)];
  if (!a.first) {
#pragma unroll
    for (int j = 0; j < KB; ++j) f.old[j] = S[p * a.D + sgm_min(d0 + j, a.D - 1)];
  }
}

template <int KB>
__global__ __launch_bounds__(DCA_WAVE) void sgm_path_kernel(const u64* __restrict__ census, unsigned short* S, SgmScan a) {
  const int lane = threadIdx.x, line = blockIdx.x, H = a.H, W = a.W, D = a.D, d0 = lane * KB;
  const u64* cL = census;
  const u64* cR = census + (long)H * W;
  const int steps = a.dy == 0 ? W : H;
  int y = a.dy == 0 ? line : (a.dy > 0 ? 0 : H - 1);
  int x = a.dy == 0 ? (a.dx > 0 ? 0 : W - 1) : line;
  bool reset = true;                                         // the predecessor of (y, x) lies outside the image
  int L[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) L[j] = SGM_NONE;
  SgmFetch<KB> cur, nxt;
  sgm_fetch<KB>(cL, cR, S, a, y, x, d0, cur);
  nxt = cur;
  for (int t = 0; t < steps; ++t) {
    int ny = y + a.dy, nx = x + a.dx;
    bool nreset = false;
    if (nx >= W) nx = 0, nreset = a.dy != 0;                 // (a horizontal scan ends here: t + 1 == steps)
    if (nx < 0) nx = W - 1, nreset = a.dy != 0;
    if (t + 1 < steps) sgm_fetch<KB>(cL, cR, S, a, ny, nx, d0, nxt);

    int c[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) c[j] = x - (d0 + j) >= 0 ? (int)__popcll(cur.cl ^ cur.cr[j]) : SGM_COST_OUT;
    if (reset) {
#pragma unroll
      for (int j = 0; j < KB; ++j) L[j] = d0 + j < D ? c[j] : SGM_NONE;
    } else {
      int m = L[0];
#pragma unroll
      for (int j = 1; j < KB; ++j) m = sgm_min(m, L[j]);
      m = sgm_wave_min(m);
      int lo = __shfl_up(L[KB - 1], 1, DCA_WAVE), hi = __shfl_down(L[0], 1, DCA_WAVE);
      lo = lane == 0 ? SGM_NONE : lo;
      hi = lane == DCA_WAVE - 1 ? SGM_NONE : hi;
      int nl[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int lm = j > 0 ? L[j - 1] : lo, lp = j < KB - 1 ? L[j + 1] : hi;
        nl[j] = d0 + j < D ? sgm_step(c[j], L[j], lm, lp, m, a.P1, a.P2) : SGM_NONE;
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) L[j] = nl[j];
    }
    unsigned short* out = S + ((long)y * W + x) * D;
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (d0 + j < D) out[d0 + j] = (unsigned short)(a.first ? L[j] : (int)cur.old[j] + L[j]);
    cur = nxt, y = ny, x = nx, reset = nreset;
  }
}

// ---- 3. winner-take-all: grid ceil(H W / 4), one wave per pixel --------------------------------------------------------------
struct SgmWta {
  int H, W, D, uniqueness, min_disp;
  float* disp;
  float* valid;
  int* cost;
  float* disp_right;
  float* disp_right_mirrored;
};

template <bool RIGHT>
__global__ __launch_bounds__(SGM_WTA_THREADS) void sgm_wta_kernel(const unsigned short* __restrict__ S, SgmWta a) {
  const int lane = threadIdx.x & (DCA_WAVE - 1), W = a.W, D = a.D;
  const long pix = (long)blockIdx.x * (SGM_WTA_THREADS / DCA_WAVE) + (threadIdx.x >> 6);
  if (pix >= (long)a.H * W) return;                          // the whole wave
  const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
  const int nk = RIGHT ? sgm_min(D, W - x) : D;              // the bins present
  auto at = [&](int k) -> int { return RIGHT ? S[(pix + k) * D + k] : S[pix * D + k]; };      // x + k < W: the same row
  int v[DCA_SGM_MAX_DISP / DCA_WAVE];
  unsigned key = ~0u;
#pragma unroll
  for (int j = 0; j < DCA_SGM_MAX_DISP / DCA_WAVE; ++j) {
    const int k = lane + DCA_WAVE * j;
    v[j] = SGM_NONE;
    if (k < nk) {
      v[j] = at(k);
      const unsigned cand = (unsigned)v[j] << 9 | (unsigned)k;
      key = cand < key ? cand : key;
    }
  }
#pragma unroll
  for (int o = DCA_WAVE / 2; o > 0; o >>= 1) {
    const unsigned other = __shfl_xor(key, o, DCA_WAVE);
    key = other < key ? other : key;
  }
  const int ds = (int)(key & 511u), s = (int)(key >> 9);
  int off = 0;
  if (ds > 0 && ds < nk - 1) off = sgm_subpixel(at(ds - 1), s, at(ds + 1));
  const float d = (float)(16 * ds + off) / 16.0f;
  if (RIGHT) {
    if (lane == 0) {
      if (a.disp_right) a.disp_right[pix] = d;
      if (a.disp_right_mirrored) a.disp_right_mirrored[(long)y * W + (W - 1 - x)] = d;
    }
  } else {
    int other = SGM_NONE;
#pragma unroll
    for (int j = 0; j < DCA_SGM_MAX_DISP / DCA_WAVE; ++j) {
      const int k = lane + DCA_WAVE * j;
      if (k < nk && (k < ds - 1 || k > ds + 1)) other = sgm_min(other, v[j]);
    }
    other = sgm_wave_min(other);
    const bool ok = sgm_unique(s, other, a.uniqueness) && ds >= a.min_disp;
    if (lane == 0) {
      if (a.disp) a.disp[pix] = ok ? d : 0.f;
      if (a.valid) a.valid[pix] = ok ? 1.f : 0.f;
      if (a.cost) a.cost[pix] = s;
    }
  }
}

inline bool sgm_dims_ok(int H, int W, int D) {
  return H >= DCA_SGM_MIN_DIM && H <= DCA_SGM_MAX_DIM && W >= DCA_SGM_MIN_DIM && W <= DCA_SGM_MAX_DIM && D >= DCA_SGM_MIN_DISP &&
         D <= DCA_SGM_MAX_DISP && (long)H * W * D < (1L << 30);
}

inline void sgm_launch_census(const unsigned char* left, const unsigned char* right, u64* census, int H, int W, int C,
                              hipStream_t stream) {
  hipLaunchKernelGGL(sgm_census_kernel, dim3((unsigned)cdiv(W, SGM_TILE_W), (unsigned)cdiv(H, SGM_TILE_H), 2u),
                     dim3(SGM_TILE_W * SGM_TILE_H), 0, stream, left, right, census, H, W, C);
}

}  // namespace

extern "C" long dca_sgm_workspace_bytes(int H, int W, int max_disp) {
  if (!sgm_dims_ok(H, W, max_disp)) return -1;
  return 16L * H * W + 2L * H * W * max_disp;
}

extern "C" int dca_sgm_census(const unsigned char* left, const unsigned char* right, unsigned long long* census, int H, int W,
                              int C, hipStream_t stream) {
  DCA_REQUIRE(left && right && census && ((uintptr_t)census & 7) == 0 && (C == 1 || C == 3 || C == 4));
  DCA_REQUIRE(sgm_dims_ok(H, W, DCA_SGM_MIN_DISP));
  sgm_launch_census(left, right, census, H, W, C, stream);
  return dca_launch_status();
}

extern "C" int dca_sgm_disparity(const unsigned char* left, const unsigned char* right, void* workspace, float* disp,
                                 float* valid, int* cost, float* disp_right, float* disp_right_mirrored, int H, int W, int C,
                                 int max_disp, int paths, int P1, int P2, int uniqueness, int min_disp, hipStream_t stream) {
  const int D = max_disp;
  DCA_REQUIRE(left && right && workspace && ((uintptr_t)workspace & 7) == 0 && (C == 1 || C == 3 || C == 4));
  DCA_REQUIRE(sgm_dims_ok(H, W, D) && (paths == 4 || paths == 8));
  DCA_REQUIRE(P1 >= 1 && P1 <= P2 && P2 <= DCA_SGM_MAX_P && uniqueness >= 0 && uniqueness <= 99 && min_disp >= 0 && min_disp < D);
  const bool left_view = disp || valid || cost, right_view = disp_right || disp_right_mirrored;
  DCA_REQUIRE(left_view || right_view);
  DCA_REQUIRE(((uintptr_t)disp & 3) == 0 && ((uintptr_t)valid & 3) == 0 && ((uintptr_t)cost & 3) == 0 &&
              ((uintptr_t)disp_right & 3) == 0 && ((uintptr_t)disp_right_mirrored & 3) == 0);
  u64* census = (u64*)workspace;
  unsigned short* S = (unsigned short*)(census + 2L * H * W);
  sgm_launch_census(left, right, census, H, W, C, stream);
  static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};      // (dy, dx)
  for (int i = 0; i < paths; ++i) {
    const SgmScan a = {H, W, D, P1, P2, dirs[i][0], dirs[i][1], i == 0 ? 1 : 0};
    const dim3 grid((unsigned)(a.dy == 0 ? H : W)), block(DCA_WAVE);
    switch (cdiv(D, DCA_WAVE)) {
      case 1: hipLaunchKernelGGL(sgm_path_kernel<1>, grid, block, 0, stream, (const u64*)census, S, a); break;
      case 2: hipLaunchKernelGGL(sgm_path_kernel<2>, grid, block, 0, stream, (const u64*)census, S, a); break;
      case 3: hipLaunchKernelGGL(sgm_path_kernel<3>, grid, block, 0, stream, (const u64*)census, S, a); break;
      default: hipLaunchKernelGGL(sgm_path_kernel<4>, grid, block, 0, stream, (const u64*)census, S, a); break;
    }
  }
  const SgmWta w = {H, W, D, uniqueness, min_disp, disp, valid, cost, disp_right, disp_right_mirrored};
  const dim3 grid((unsigned)cdiv((long)H * W, SGM_WTA_THREADS / DCA_WAVE)), block(SGM_WTA_THREADS);
  if (left_view) hipLaunchKernelGGL(sgm_wta_kernel<false>, grid, block, 0, stream, (const unsigned short*)S, w);
  if (right_view) hipLaunchKernelGGL(sgm_wta_kernel<true>, grid, block, 0, stream, (const unsigned short*)S, w);
  return dca_launch_status();
}
