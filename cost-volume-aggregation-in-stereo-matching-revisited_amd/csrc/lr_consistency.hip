// Left-right consistency of a disparity pair (inference only; nothing in the reference computes it).
// In a half-occluded region -- the band to the left of every foreground object, the left image border -- the network has
// nothing to match and the soft-argmin there is often sharp and wrong, so the confidence of section 6e does not flag it.
// The standard answer is the cross-check: estimate the right view's disparity, compare, invalidate and fill.
//
//  * mirror_pair -- (left, right) -> (flipW(right), flipW(left)), one launch, bit copies.  On this pair the UNCHANGED
//    network computes the right view's disparity in mirrored coordinates: with R'(x) = R(W-1-x), L'(x) = L(W-1-x),
//    corr(R'(x), L'(x-d)) = corr(R(u), L(u+d)) at u = W-1-x.
//  * lr_consistency -- one workgroup per image row: the rows of both disparity maps are staged in LDS (the right one
//    un-mirrored on the way in), every left pixel looks its disparity up in the right map (linear interpolation), and the
//    invalid ones are filled from the nearest valid neighbours in the row as the KITTI devkit's background interpolation
//    does.  "Nearest valid to the left / right" is a prefix-max of (valid ? x : -1) and a suffix-min of (valid ? x : cols):
//    serial over a thread's own run of columns (a 32-bit mask), __shfl_up / __shfl_down across the 64 lanes, LDS across
//    the four waves.  Everything after the comparison is integer arithmetic or a copy of an input value: order-free and
//    bitwise reproducible.  Global loads and stores are coalesced over x; the run-wise passes touch LDS only.
#include "dca_common.h"
#include "../../include/dca_hip.h"

// the formulas of include/dca_hip.h as they are written: no contraction into fma
#pragma clang fp contract(off)

namespace {

#define LR_THREADS 256
#define LR_WAVES (LR_THREADS / DCA_WAVE)

// ---- (a) the mirrored, swapped pair ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(LR_THREADS) void mirror_pair_kernel(const unsigned* __restrict__ left,
                                                                 const unsigned* __restrict__ right,
                                                                 unsigned* __restrict__ out_left,
                                                                 unsigned* __restrict__ out_right, long total, int W) {
  for (long idx = (long)blockIdx.x * LR_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * LR_THREADS) {
    const long row = idx / W;
    const long src = row * W + (W - 1 - (int)(idx - row * W));
    out_left[idx] = right[src];
    out_right[idx] = left[src];
  }
}

// ---- (b) cross-check, invalidation, fill -----------------------------------------------------------------------------------
// LDS: sD[W] = the row of dl; sR[W] = the row of the right disparity in its own coordinates, sR[i] = drm[W-1-i].  Once the
// cross-check has read it, sR is reused: first for the validity flags (column-wise -> run-wise hand-over), then for the
// filled row (run-wise -> column-wise hand-over).
__global__ __launch_bounds__(LR_THREADS) void lr_consistency_kernel(const float* __restrict__ dl,
                                                                    const float* __restrict__ drm,
                                                                    float* __restrict__ diff, float* __restrict__ valid,
                                                                    float* __restrict__ filled,
                                                                    float* __restrict__ disp_right, int W, int cols,
                                                                    int run, float tau) {
  extern __shared__ float lr_lds[];
  __shared__ int wave_last[LR_WAVES], wave_first[LR_WAVES];
  float* sD = lr_lds;
  float* sR = lr_lds + W;
  const int t = threadIdx.x;
  const long base = (long)blockIdx.x * W;
  for (int x = t; x < W; x += LR_THREADS) {
    sD[x] = dl[base + x];
    sR[x] = drm[base + (W - 1 - x)];
  }
  __syncthreads();

  // column-wise: thread t owns x = t + 256 j, j < 32 (W <= 8192); bit j of vmask = valid
  unsigned vmask = 0;
  for (int x = t, j = 0; x < W; x += LR_THREADS, ++j) {
    float df = INFINITY;
    if (x < cols) {
      const float d = sD[x];
      const float xr = (float)x - d;
      if (d > 0.f && xr >= 0.f) {                       // in view; xr <= x < cols, so 0 <= i0 <= cols - 1
        const float fl = floorf(xr);
        const int i0 = (int)fl;
        const int i1 = i0 + 1 < cols ? i0 + 1 : cols - 1;
        const float f = xr - fl;
        const float r = (1.f - f) * sR[i0] + f * sR[i1];
        df = fabsf(d - r);
      }
    }
    const bool ok = df <= tau;                          // NaN: false
    vmask |= ok ? 1u << j : 0u;
    if (diff) diff[base + x] = df;
    valid[base + x] = ok ? 1.f : 0.f;
    if (disp_right) disp_right[base + x] = sR[x];
  }
  if (!filled) return;                                  // uniform: a kernel argument
  __syncthreads();                                      // every look-up into sR is done
  for (int x = t, j = 0; x < cols; x += LR_THREADS, ++j) sR[x] = __uint_as_float((vmask >> j) & 1u);
  __syncthreads();

  // run-wise: thread t owns the columns [x0, x1) of [0, cols), at most 32; bit j of mask = valid(x0 + j)
  const int x0 = t * run < cols ? t * run : cols;
  const int x1 = x0 + run < cols ? x0 + run : cols;
  unsigned mask = 0;
  for (int x = x0; x < x1; ++x) mask |= __float_as_uint(sR[x]) << (x - x0);
  const int lane = t & (DCA_WAVE - 1), wave = t / DCA_WAVE;
  int last = mask ? x0 + 31 - __clz((int)mask) : -1;          // inclusive prefix-max over the lanes
  int first = mask ? x0 + __ffs((int)mask) - 1 : cols;        // inclusive suffix-min
#pragma unroll
  for (int o = 1; o < DCA_WAVE; o <<= 1) {
    const int a = __shfl_up(last, o, DCA_WAVE), b = __shfl_down(first, o, DCA_WAVE);
    last = lane >= o && a > last ? a : last;
    first = lane + o < DCA_WAVE && b < first ? b : first;
  }
  if (lane == DCA_WAVE - 1) wave_last[wave] = last;
  if (lane == 0) wave_first[wave] = first;
  int lcarry = __shfl_up(last, 1, DCA_WAVE), rcarry = __shfl_down(first, 1, DCA_WAVE);     // exclusive, within the wave
  lcarry = lane > 0 ? lcarry : -1;
  rcarry = lane < DCA_WAVE - 1 ? rcarry : cols;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < LR_WAVES; ++w) {
    const int a = wave_last[w], b = wave_first[w];
    lcarry = w < wave && a > lcarry ? a : lcarry;
    rcarry = w > wave && b < rcarry ? b : rcarry;
  }
  for (int x = x0; x < x1; ++x) {
    const int j = x - x0;
    float v = sD[x];
    if (!((mask >> j) & 1u)) {
      const unsigned lm = mask & ((1u << j) - 1u), rm = (mask >> j) >> 1;
      const int l = lm ? x0 + 31 - __clz((int)lm) : lcarry;
      const int r = rm ? x + __ffs((int)rm) : rcarry;
      if (l >= 0 && r < cols) {
        const float a = sD[l], b = sD[r];                     // valid pixels: never NaN
        v = b < a ? b : a;
      } else if (l >= 0) {
        v = sD[l];
      } else if (r < cols) {
        v = sD[r];
      }
    }
    sR[x] = v;                                                // the thread's own run: nobody else reads or writes it here
  }
  __syncthreads();
  for (int x = t; x < W; x += LR_THREADS) filled[base + x] = x < cols ? sR[x] : sD[x];
}

}  // namespace

extern "C" int dca_mirror_pair(const float* left, const float* right, float* out_left, float* out_right, int N, int H, int W,
                               hipStream_t stream) {
  DCA_REQUIRE(left && right && out_left && out_right && N > 0 && H > 0 && W > 0);
  DCA_REQUIRE(out_left != left && out_left != right && out_right != left && out_right != right && out_left != out_right);
  const long total = (long)N * H * W, g = (total + LR_THREADS - 1) / LR_THREADS;
  hipLaunchKernelGGL(mirror_pair_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(LR_THREADS), 0, stream,
                     (const unsigned*)left, (const unsigned*)right, (unsigned*)out_left, (unsigned*)out_right, total, W);
  return dca_launch_status();
}

extern "C" int dca_lr_consistency(const float* dl, const float* drm, float* diff, float* valid, float* filled,
                                  float* disp_right, int B, int H, int W, int cols, float tau, hipStream_t stream) {
  DCA_REQUIRE(dl && drm && valid && B > 0 && H > 0 && W > 0 && W <= DCA_LR_MAX_W && (long)B * H < (1L << 31));
  DCA_REQUIRE(cols >= 1 && cols <= W);
  DCA_REQUIRE(tau >= 0.f && tau < INFINITY);            // NaN fails both; +inf would make out-of-view pixels valid
  const int run = (cols + LR_THREADS - 1) / LR_THREADS;                // <= 32
  const size_t lds = (size_t)2 * W * sizeof(float);
  if (lds + 256 > 64 * 1024) {                                         // + the static words of the wave hand-over
    hipError_t e = hipFuncSetAttribute((const void*)lr_consistency_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(lr_consistency_kernel, dim3((unsigned)((long)B * H)), dim3(LR_THREADS), lds, stream, dl, drm, diff,
                     valid, filled, disp_right, W, cols, run, tau);
  return dca_launch_status();
}
static_assert(DCA_LR_MAX_W <= 32 * LR_THREADS, "one mask bit per column of a thread's run");
