// Sparse ground truth from a LiDAR scan (nothing in the reference computes it): the points of one
// scan, already on the device, projected into the rectified left image -> a sparse disparity map, metric depth and the
// KITTI uint16 encoding, the definitions of include/dca_hip.h (dca_lidar_disparity) as they are written.
//
//  1. fill:    the z-buffer becomes the bits of +inf everywhere, the two counters 0;
//  2. scatter: one thread per point projects it and, if it is kept, takes the INTEGER atomicMin of its depth's bit pattern
//              into the pixel's word.  Depths are positive, so their bits order as the floats do, and a minimum is the same
//              whatever the order of arrival: no float atomics, bitwise reproducible.  The word only ever decreases, so a
//              plain load that already shows a smaller value lets the thread skip its atomic;
//  3. resolve: a workgroup stages an LD_TW x LD_TH tile with its halo in LDS, takes the window minimum along rows, then
//              along columns (2 rx + 2 ry + 2 LDS reads per pixel, not (2 rx + 1)(2 ry + 1) global ones), and writes the
//              outputs; eight workgroups per CU (all it holds) walk the tiles.
// The two counters take integer atomicAdds, one per workgroup.
// Kernel boundaries are the only global synchronisation.  ~2 MB of points and a z-buffer that fits in L2: the three
// launches are latency-bound, the kernels are kept plain.
#include "dca_common.h"
#include "../../include/dca_hip.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define LD_THREADS 256
#define LD_TW 32
#define LD_TH 8
#define LD_R DCA_LIDAR_MAX_RADIUS
#define LD_INF 0x7f800000u                               // the bits of +inf: above every finite positive float's
// a tile with the largest halo, in steps of the tile's own rows and columns
#define LD_HALO_A ((LD_TH + 2 * LD_R + LD_TH - 1) / LD_TH)
#define LD_HALO_B ((LD_TW + 2 * LD_R + LD_TW - 1) / LD_TW)
static_assert(LD_TW * LD_TH == LD_THREADS && LD_THREADS % DCA_WAVE == 0, "one thread per tile pixel, whole waves");

struct LidarProj {
  float m[12];
  int H, W;
  float min_depth, max_depth;
};

// the wave totals of a workgroup (the same number in every lane of a wave: a ballot's population count) -> ONE integer
// atomicAdd.  Thousands of atomics on one address serialise (33 us for the 7332 waves of a KITTI frame, DESIGN.md section
// 6k); a sum of integers does not depend on their order.  Every thread of the workgroup must call it.
__device__ __forceinline__ void block_add(unsigned long long* counter, unsigned wave_total) {
  __shared__ unsigned totals[LD_THREADS / DCA_WAVE];
  if ((threadIdx.x & (DCA_WAVE - 1)) == 0) totals[threadIdx.x / DCA_WAVE] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < LD_THREADS / DCA_WAVE; ++w) sum += totals[w];
    if (sum) atomicAdd(counter, (unsigned long long)sum);
  }
}

__global__ __launch_bounds__(LD_THREADS) void lidar_fill_kernel(unsigned* __restrict__ zbuf, long hw,
                                                                unsigned long long* __restrict__ count) {
  for (long i = (long)blockIdx.x * LD_THREADS + threadIdx.x; i < hw; i += (long)gridDim.x * LD_THREADS) zbuf[i] = LD_INF;
  if (count && blockIdx.x == 0 && threadIdx.x < 2) count[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(LD_THREADS) void lidar_scatter_kernel(const float* __restrict__ points, int S, long n, LidarProj a,
                                                                   unsigned* __restrict__ zbuf,
                                                                   unsigned long long* __restrict__ count) {
  const long i = (long)blockIdx.x * LD_THREADS + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const float* p = points + i * S;
    const float X = p[0], Y = p[1], Z = p[2];
    const float x = ((a.m[0] * X + a.m[1] * Y) + a.m[2] * Z) + a.m[3];
    const float y = ((a.m[4] * X + a.m[5] * Y) + a.m[6] * Z) + a.m[7];
    const float z = ((a.m[8] * X + a.m[9] * Y) + a.m[10] * Z) + a.m[11];
    const float u = x / z, v = y / z;
    const float uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
    // in float, before any conversion: a NaN fails, +-inf and 1e30 fail without overflowing an int
    keep = z >= a.min_depth && z <= a.max_depth && uf >= 0.f && uf < (float)a.W && vf >= 0.f && vf < (float)a.H;
    if (keep) {
      unsigned* word = zbuf + ((long)(int)vf * a.W + (int)uf);
      const unsigned bits = __float_as_uint(z);          // z >= min_depth > 0: the bits order as the floats
      if (*word > bits) atomicMin(word, bits);           // the word only decreases: a smaller value seen stays smaller
    }
  }
  if (count) block_add(count + 1, (unsigned)__popcll(__ballot(keep)));
}

struct LidarOut {
  float* disp;
  float* depth;
  unsigned short* disp_u16;
  unsigned long long* count;
  float fb, doffs, min_disp, max_disp, occl_scale;
};

// persistent: a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... and adds its pixel count once at the end
__global__ __launch_bounds__(LD_THREADS) void lidar_resolve_kernel(const unsigned* __restrict__ zbuf, int H, int W, int tiles_x,
                                                                   int tiles, int rx, int ry, LidarOut o) {
  __shared__ unsigned tile[LD_TH + 2 * LD_R][LD_TW + 2 * LD_R];      // the tile of zbuf with its halo; +inf outside the image
  __shared__ unsigned rowmin[LD_TH + 2 * LD_R][LD_TW];               // minimum over columns c-rx .. c+rx of every halo row
  const int t = threadIdx.x;
  const int hh = LD_TH + 2 * ry, hw = LD_TW + 2 * rx;               // rx, ry <= LD_R: inside the arrays
  const int lr = t / LD_TW, lc = t - lr * LD_TW;
  unsigned written = 0;                                             // of this wave, over all its tiles
  for (int id = blockIdx.x; id < tiles; id += gridDim.x) {
    const int ty0 = (id / tiles_x) * LD_TH, tx0 = (id % tiles_x) * LD_TW;
    // thread (lr, lc) stages the halo words (lr + 8 a, lc + 32 b): no division, and every load of the thread is issued before
    // the first one is waited for (a loop with a run-time trip count waits for each in turn)
    unsigned halo[LD_HALO_A][LD_HALO_B];
#pragma unroll
    for (int a = 0; a < LD_HALO_A; ++a) {
#pragma unroll
      for (int b = 0; b < LD_HALO_B; ++b) {
        const int hr = lr + a * LD_TH, hc = lc + b * LD_TW;
        const int r = ty0 - ry + hr, c = tx0 - rx + hc;
        halo[a][b] = (hr < hh && hc < hw && r >= 0 && r < H && c >= 0 && c < W) ? zbuf[(long)r * W + c] : LD_INF;
      }
    }
#pragma unroll
    for (int a = 0; a < LD_HALO_A; ++a) {
#pragma unroll
      for (int b = 0; b < LD_HALO_B; ++b) {
        const int hr = lr + a * LD_TH, hc = lc + b * LD_TW;
        if (hr < hh && hc < hw) tile[hr][hc] = halo[a][b];
      }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < LD_HALO_A; ++a) {
      const int hr = lr + a * LD_TH;
      if (hr < hh) {
        unsigned m = tile[hr][lc];
        for (int k = 1; k <= 2 * rx; ++k) m = min(m, tile[hr][lc + k]);
        rowmin[hr][lc] = m;
      }
    }
    __syncthreads();
    unsigned m = rowmin[lr][lc];
    for (int k = 1; k <= 2 * ry; ++k) m = min(m, rowmin[lr + k][lc]);
    const unsigned zb = tile[lr + ry][lc + rx];
    const int r = ty0 + lr, c = tx0 + lc;
    const bool inside = r < H && c < W;
    const float z = __uint_as_float(zb), zmin = __uint_as_float(m);
    const float d = o.fb / z - o.doffs;
    const bool valid = inside && zb != LD_INF && z <= zmin * o.occl_scale && d >= o.min_disp && d < o.max_disp;
    if (inside) {
      const long at = (long)r * W + c;
      if (o.disp) o.disp[at] = valid ? d : 0.f;
      if (o.depth) o.depth[at] = valid ? z : 0.f;
      if (o.disp_u16) {
        const float q = d * 256.0f + 0.5f;
        o.disp_u16[at] = !valid ? 0 : q >= 65535.f ? 65535 : q >= 1.f ? (unsigned short)(unsigned)q : 1;
      }
    }
    written += (unsigned)__popcll(__ballot(valid));
    __syncthreads();                                                // tile and rowmin are rewritten by the next tile
  }
  if (o.count) block_add(o.count, written);
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }

}  // namespace

extern "C" int dca_lidar_disparity(const float* points, long N, int S, long n, float m00, float m01, float m02, float m03,
                                   float m10, float m11, float m12, float m13, float m20, float m21, float m22, float m23, int H,
                                   int W, float fb, float doffs, float min_depth, float max_depth, float min_disp,
                                   float max_disp, int rx, int ry, double rel, float* disp, float* depth,
                                   unsigned short* disp_u16, long long* count, unsigned* zbuf, hipStream_t stream) {
  DCA_REQUIRE(N >= 0 && n >= 0 && n <= N && S >= 3 && n < (1L << 31) && n * (long)S < (1L << 31) && (points || n == 0));
  DCA_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31));
  DCA_REQUIRE(rx >= 0 && rx <= DCA_LIDAR_MAX_RADIUS && ry >= 0 && ry <= DCA_LIDAR_MAX_RADIUS);
  DCA_REQUIRE(rel >= 0.0 && rel < (double)INFINITY);
  DCA_REQUIRE(min_depth > 0.f && max_depth >= min_depth && max_depth < INFINITY);
  DCA_REQUIRE(finite_f(min_disp) && finite_f(max_disp) && max_disp >= min_disp);
  DCA_REQUIRE(fb > 0.f && fb < INFINITY && finite_f(doffs));
  DCA_REQUIRE(disp || depth || disp_u16 || count);
  DCA_REQUIRE(zbuf && ((uintptr_t)zbuf & 3) == 0 && ((uintptr_t)count & 7) == 0);
  const LidarProj a = {{m00, m01, m02, m03, m10, m11, m12, m13, m20, m21, m22, m23}, H, W, min_depth, max_depth};
  for (int i = 0; i < 12; ++i) DCA_REQUIRE(finite_f(a.m[i]));
  const LidarOut o = {disp, depth, disp_u16, (unsigned long long*)count, fb, doffs, min_disp, max_disp, (float)(1.0 + rel)};
  const long hw = (long)H * W;
  long fill = (hw + LD_THREADS - 1) / LD_THREADS;
  fill = fill > 2048 ? 2048 : fill;
  const long scatter = n > 0 ? (n + LD_THREADS - 1) / LD_THREADS : 1;
  const int tiles_x = cdiv(W, LD_TW);
  const long tiles = (long)tiles_x * cdiv(H, LD_TH);
  hipLaunchKernelGGL(lidar_fill_kernel, dim3((unsigned)fill), dim3(LD_THREADS), 0, stream, zbuf, hw, o.count);
  hipLaunchKernelGGL(lidar_scatter_kernel, dim3((unsigned)scatter), dim3(LD_THREADS), 0, stream, points, S, n, a, zbuf, o.count);
  const long resolve = tiles < 8L * dca_num_cus() ? tiles : 8L * dca_num_cus();      // 8 x 4 waves: what a CU holds
  hipLaunchKernelGGL(lidar_resolve_kernel, dim3((unsigned)resolve), dim3(LD_THREADS), 0, stream, (const unsigned*)zbuf, H, W,
                     tiles_x, (int)tiles, rx, ry, o);
  return dca_launch_status();
}
