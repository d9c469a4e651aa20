// Geometry from calibrated disparity (inference only; nothing in the reference computes it): the
// metric depth map and a compacted, coloured point cloud in the camera frame, from maps that are already in device memory
// when the disparity appears -- the prediction, the confidence or left-right validity map, the uint8 source image.
//
//  * disp_to_depth -- one launch: Z = f b / (d + doffs) where the pixel passes the filters, +0.0 elsewhere, as fp32 and / or
//    uint16(Z * scale).
//  * point_cloud -- stream compaction in THREE launches, kernel boundaries being the only global synchronisation:
//      1. count: one workgroup per tile of DCA_PC_TILE pixels counts its kept pixels (wave ballot + population count);
//      2. scan:  ONE workgroup turns the tile counts into exclusive offsets, 256 at a time with a carry, and writes the totals;
//      3. emit:  one workgroup per tile evaluates the predicate again, ranks its kept pixels (ballot + mbcnt within the
//                wave, a scan of the wave totals in LDS within the tile) and writes the 16-byte records below `cap`.
//    No atomics, so the records and their ORDER (row-major window order) are bitwise reproducible.  No single-pass scan
//    with look-back and no cooperative launch: a workgroup that polls a flag of one that is not resident hangs the queue.
//    Re-evaluating the predicate costs a second read of pred and mask (8 B per pixel) and saves a 1 B/pixel flag round
//    trip plus its layout; the kernels are launch-bound at KITTI size either way.
//
// A tile is walked in PC_PASSES passes of PC_THREADS consecutive pixels: consecutive lanes take consecutive window indices
// (coalesced loads of pred and mask), and a tile is PC_GROUPS = passes x waves groups of 64 consecutive pixels, ranked in
// that order.
#include "dca_common.h"
#include "../../include/dca_hip.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / DCA_WAVE)
#define PC_PASSES (DCA_PC_TILE / PC_THREADS)
#define PC_GROUPS (PC_PASSES * PC_WAVES)
static_assert(DCA_PC_TILE % PC_THREADS == 0 && PC_THREADS % DCA_WAVE == 0, "a tile is whole passes of whole waves");

struct GeoArgs {
  const float* pred;           // (Hc,Wc)
  const float* mask;           // (Hc,Wc) or NULL
  int Wc, y0, rows, cols, stride;
  float fb, doffs, min_disp, max_depth, mask_min;
};

// THE predicate: window pixel i = r cols + c -> kept or not, and its depth.  NaN fails every comparison.
__device__ __forceinline__ bool geo_keep(const GeoArgs& a, int i, int& r, int& c, float& Z) {
  r = i / a.cols;
  c = i - r * a.cols;
  const long at = (long)(a.y0 + r) * a.Wc + c;
  const float d = a.pred[at];
  const float den = d + a.doffs;
  Z = a.fb / den;
  bool keep = d >= a.min_disp && den > 0.f && Z > 0.f && Z <= a.max_depth;
  if (a.mask) keep = keep && a.mask[at] >= a.mask_min;
  return keep && r % a.stride == 0 && c % a.stride == 0;
}

__global__ __launch_bounds__(PC_THREADS) void disp_to_depth_kernel(GeoArgs a, float* __restrict__ out_f32,
                                                                   unsigned short* __restrict__ out_u16, float scale) {
  const int n = a.rows * a.cols;
  for (long i = (long)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PC_THREADS) {
    int r, c;
    float Z;
    const float z = geo_keep(a, (int)i, r, c, Z) ? Z : 0.f;
    if (out_f32) out_f32[i] = z;
    if (out_u16) out_u16[i] = dca_sat_u16(z * scale);
  }
}

__device__ __forceinline__ unsigned popc64(unsigned long long b) { return (unsigned)__popcll(b); }

// ---- 1. kept pixels per tile -> counts[tile] ---------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(GeoArgs a, unsigned* __restrict__ counts) {
  __shared__ unsigned wave_total[PC_WAVES];
  const int n = a.rows * a.cols, t = threadIdx.x;
  const long base = (long)blockIdx.x * DCA_PC_TILE;
  unsigned mine = 0;                                     // lane 0 of every wave: the wave's kept pixels over all passes
#pragma unroll
  for (int p = 0; p < PC_PASSES; ++p) {
    const long i = base + p * PC_THREADS + t;
    int r, c;
    float Z;
    const bool keep = i < n && geo_keep(a, (int)i, r, c, Z);
    mine += popc64(__ballot(keep));
  }
  if ((t & (DCA_WAVE - 1)) == 0) wave_total[t / DCA_WAVE] = mine;
  __syncthreads();
  if (t == 0) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < PC_WAVES; ++w) s += wave_total[w];
    counts[blockIdx.x] = s;
  }
}

// ---- 2. exclusive scan of the tile counts, in place; ONE workgroup, PC_THREADS tiles per step with a carry -----------------
__global__ __launch_bounds__(PC_THREADS) void pc_scan_kernel(unsigned* __restrict__ offs, long long* __restrict__ count,
                                                             int tiles, long cap) {
  __shared__ unsigned wave_total[PC_WAVES];
  const int t = threadIdx.x, lane = t & (DCA_WAVE - 1), wave = t / DCA_WAVE;
  unsigned carry = 0;                                    // the total stays below 2^31: at most rows cols
  for (int b = 0; b < tiles; b += PC_THREADS) {
    const unsigned v = b + t < tiles ? offs[b + t] : 0u;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < DCA_WAVE; o <<= 1) {
      const unsigned up = __shfl_up(incl, o, DCA_WAVE);
      incl += lane >= o ? up : 0u;
    }
    if (lane == DCA_WAVE - 1) wave_total[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PC_WAVES; ++w) {
      const unsigned s = wave_total[w];
      before += w < wave ? s : 0u;
      all += s;
    }
    if (b + t < tiles) offs[b + t] = carry + before + incl - v;
    carry += all;
    __syncthreads();                                     // wave_total is rewritten by the next step
  }
  if (t == 0) {
    offs[tiles] = carry;
    count[0] = (long long)carry;
    count[1] = (long long)carry < (long long)cap ? (long long)carry : (long long)cap;
  }
}

// ---- 3. the records ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_THREADS) void pc_emit_kernel(GeoArgs a, const unsigned* __restrict__ offs,
                                                             const unsigned char* __restrict__ rgb, int C, int Wsrc, int v0,
                                                             float f, float cx, float cy, uint4* __restrict__ vertices,
                                                             long cap) {
  __shared__ unsigned group_total[PC_GROUPS];
  const int n = a.rows * a.cols, t = threadIdx.x, lane = t & (DCA_WAVE - 1), wave = t / DCA_WAVE;
  const long base = (long)blockIdx.x * DCA_PC_TILE;
  bool keep[PC_PASSES];
  int r[PC_PASSES], c[PC_PASSES];
  float Z[PC_PASSES];
  unsigned below[PC_PASSES];                             // kept pixels of the same group on lower lanes
#pragma unroll
  for (int p = 0; p < PC_PASSES; ++p) {
    const long i = base + p * PC_THREADS + t;
    keep[p] = i < n && geo_keep(a, (int)i, r[p], c[p], Z[p]);
    const unsigned long long b = __ballot(keep[p]);
    below[p] = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    if (lane == 0) group_total[p * PC_WAVES + wave] = popc64(b);
  }
  __syncthreads();
  const long tile_first = offs[blockIdx.x];
  unsigned run = 0;                                      // kept pixels of the groups before group g, g ascending
#pragma unroll
  for (int p = 0; p < PC_PASSES; ++p) {
#pragma unroll
    for (int w = 0; w < PC_WAVES; ++w) {
      if (w == wave && keep[p]) {
        const long k = tile_first + run + below[p];
        if (k < cap) {
          const float X = (((float)c[p] - cx) * Z[p]) / f;
          const float Y = (((float)(v0 + r[p]) - cy) * Z[p]) / f;
          unsigned col = 0xffffffffu;
          if (rgb) {
            const unsigned char* px = rgb + ((long)(v0 + r[p]) * Wsrc + c[p]) * C;
            col = (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16 | 0xff000000u;
          }
          vertices[k] = make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(Z[p]), col);
        }
      }
      run += group_total[p * PC_WAVES + w];
    }
  }
}

// the scalars every kernel shares, checked once: false = refuse
bool geo_args(GeoArgs& a, const float* pred, const float* mask, int Hc, int Wc, int y0, int rows, int cols, int stride,
              float fb, float doffs, float min_disp, float max_depth, float mask_min) {
  if (!pred || !dca_window_ok(Hc, Wc, y0, rows, cols) || stride < 1) return false;
  if (!(fb > 0.f && fb < INFINITY) || !(fabsf(doffs) < INFINITY)) return false;
  if (!(min_disp >= 0.f && min_disp < INFINITY) || !(max_depth > 0.f && max_depth < INFINITY)) return false;
  if (mask && mask_min != mask_min) return false;
  a = GeoArgs{pred, mask, Wc, y0, rows, cols, stride, fb, doffs, min_disp, max_depth, mask_min};
  return true;
}

}  // namespace

extern "C" int dca_disp_to_depth(const float* pred, const float* mask, float* out_f32, unsigned short* out_u16, int Hc,
                                 int Wc, int y0, int rows, int cols, float fb, float doffs, float min_disp, float max_depth,
                                 float mask_min, float scale, hipStream_t stream) {
  GeoArgs a;
  DCA_REQUIRE(out_f32 || out_u16);
  DCA_REQUIRE(geo_args(a, pred, mask, Hc, Wc, y0, rows, cols, 1, fb, doffs, min_disp, max_depth, mask_min));
  DCA_REQUIRE(!out_u16 || (scale > 0.f && scale < INFINITY));
  long nblk = ((long)rows * cols + PC_THREADS - 1) / PC_THREADS;
  nblk = nblk > 2048 ? 2048 : nblk;
  hipLaunchKernelGGL(disp_to_depth_kernel, dim3((unsigned)nblk), dim3(PC_THREADS), 0, stream, a, out_f32, out_u16, scale);
  return dca_launch_status();
}

extern "C" long dca_point_cloud_tiles(int rows, int cols) {
  if (rows <= 0 || cols <= 0 || (long)rows * cols >= (1L << 31)) return 0;
  return ((long)rows * cols + DCA_PC_TILE - 1) / DCA_PC_TILE;
}

extern "C" int dca_point_cloud(const float* pred, const float* mask, const unsigned char* rgb, int C, int Hsrc, int Wsrc,
                               void* vertices, long cap, unsigned* tile_offsets, long long* count, int Hc, int Wc, int y0,
                               int rows, int cols, int v0, int stride, float f, float fb, float cx, float cy, float doffs,
                               float min_disp, float max_depth, float mask_min, hipStream_t stream) {
  GeoArgs a;
  DCA_REQUIRE(geo_args(a, pred, mask, Hc, Wc, y0, rows, cols, stride, fb, doffs, min_disp, max_depth, mask_min));
  DCA_REQUIRE(tile_offsets && count && cap >= 0 && (vertices || cap == 0) && ((uintptr_t)vertices & 15) == 0);
  DCA_REQUIRE(((uintptr_t)tile_offsets & 3) == 0 && ((uintptr_t)count & 7) == 0);
  DCA_REQUIRE(f > 0.f && f < INFINITY && fabsf(cx) < INFINITY && fabsf(cy) < INFINITY);
  DCA_REQUIRE(v0 >= 0 && (long)v0 + rows < (1L << 31));
  if (rgb) {
    DCA_REQUIRE((C == 3 || C == 4) && Hsrc > 0 && Wsrc > 0 && (long)Hsrc * Wsrc < (1L << 31));
    DCA_REQUIRE((long)v0 + rows <= Hsrc && cols <= Wsrc);
  }
  const long tiles = dca_point_cloud_tiles(rows, cols);
  DCA_REQUIRE(tiles > 0);
  hipLaunchKernelGGL(pc_count_kernel, dim3((unsigned)tiles), dim3(PC_THREADS), 0, stream, a, tile_offsets);
  hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(PC_THREADS), 0, stream, tile_offsets, count, (int)tiles, cap);
  hipLaunchKernelGGL(pc_emit_kernel, dim3((unsigned)tiles), dim3(PC_THREADS), 0, stream, a, (const unsigned*)tile_offsets,
                     rgb, C, Wsrc, v0, f, cx, cy, (uint4*)vertices, cap);
  return dca_launch_status();
}
