// Guided stereo (Poggi et al., CVPR 2019): sparse disparity hints modulate the cost volume.  The
// definitions of include/dca_hip.h (dca_hints_to_quarter, dca_volume_modulate) as they are written; the fused builder of
// volume_fused.hip calls the same dca_guide_factor.
//
// hints_quarter_kernel: one thread per cell of the quarter-resolution map; its 4 x 4 block of the full-resolution map is
// read through the frame's placement.  Compares and one exact multiply: bitwise what geometry.hints_to_quarter_host gives.
//
// modulate_kernel: a thread owns (b, d, y, x quad) -- or one x on the scalar path -- forms its factors once and walks the
// channels, so the volume is read and written once and a factor's expf is evaluated once, not once per channel.
#include <math.h>

#include "dca_common.h"
#include "guided_math.h"
#include "../../include/dca_hip.h"

namespace {

#define GD_THREADS 256
#define GD_MAX_BLOCKS 16384

__global__ __launch_bounds__(GD_THREADS) void hints_quarter_kernel(const float* __restrict__ hints, float* __restrict__ hints4,
                                                                   int B, int h, int w, int H4, int W4, int src_y0, int dst_y0,
                                                                   int rows, int cols, float maxdisp) {
  const long total = (long)B * H4 * W4;
  for (long idx = (long)blockIdx.x * GD_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * GD_THREADS) {
    const int X = (int)(idx % W4);
    const long t = idx / W4;
    const int Y = (int)(t % H4), b = (int)(t / H4);
    const float* src = hints + (long)b * h * w;
    float best = 0.f;
    for (int dy = 0; dy < 4; ++dy) {
      const int r = 4 * Y + dy - dst_y0;           // row of the window
      if (r < 0 || r >= rows) continue;
      for (int dx = 0; dx < 4; ++dx) {
        const int x = 4 * X + dx;
        if (x >= cols) continue;
        const float v = src[(long)(src_y0 + r) * w + x];
        if (v > 0.f && v < maxdisp && v > best) best = v;      // a NaN fails the first comparison
      }
    }
    hints4[idx] = 0.25f * best;
  }
}

// one workgroup: every thread counts the cells idx = tid, tid + 256, ..., then the partial counts are added in a fixed order
__global__ __launch_bounds__(GD_THREADS) void hints_count_kernel(const float* __restrict__ hints4, long n, long* __restrict__ count) {
  __shared__ long part[GD_THREADS];
  long c = 0;
  for (long i = threadIdx.x; i < n; i += GD_THREADS) c += hints4[i] > 0.f ? 1 : 0;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int s = GD_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = part[0];
}

// VEC: x quads and 16-byte accesses (W % 4 == 0, aligned pointers); otherwise one x per thread
template <bool VEC>
__global__ __launch_bounds__(GD_THREADS) void modulate_kernel(const float* in, const float* __restrict__ hints4, float* out, int B,
                                                              int C, int D, int H, int W, float k, float i2c2) {
  const int WX = VEC ? W >> 2 : W;
  const long HW = (long)H * W, DHW = (long)D * HW;
  const long total = (long)B * D * H * WX;
  for (long idx = (long)blockIdx.x * GD_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * GD_THREADS) {
    const int q = (int)(idx % WX);
    long t = idx / WX;
    const int y = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int b = (int)(t / D);
    const long hoff = ((long)b * H + y) * W, voff = (long)b * C * DHW + (long)d * HW + (long)y * W;
    if (VEC) {
      const int x0 = 4 * q;
      const float4 h4 = *(const float4*)(hints4 + hoff + x0);
      const float m0 = dca_guide_factor(d, h4.x, k, i2c2), m1 = dca_guide_factor(d, h4.y, k, i2c2);
      const float m2 = dca_guide_factor(d, h4.z, k, i2c2), m3 = dca_guide_factor(d, h4.w, k, i2c2);
      const float* ip = in + voff + x0;
      float* op = out + voff + x0;
#pragma unroll 4
      for (int c = 0; c < C; ++c) {
        float4 v = *(const float4*)(ip + c * DHW);
        v.x *= m0; v.y *= m1; v.z *= m2; v.w *= m3;
        *(float4*)(op + c * DHW) = v;
      }
    } else {
      const float m = dca_guide_factor(d, hints4[hoff + q], k, i2c2);
      const float* ip = in + voff + q;
      float* op = out + voff + q;
#pragma unroll 4
      for (int c = 0; c < C; ++c) op[c * DHW] = ip[c * DHW] * m;
    }
  }
}

inline int gd_blocks(long total) {
  const long blocks = (total + GD_THREADS - 1) / GD_THREADS;
  return (int)(blocks < GD_MAX_BLOCKS ? blocks : GD_MAX_BLOCKS);
}

}  // namespace

extern "C" int dca_hints_to_quarter(const float* hints, float* hints4, long* count, int B, int h, int w, int Hc, int Wc,
                                    int src_y0, int dst_y0, int rows, int cols, float maxdisp, hipStream_t stream) {
  DCA_REQUIRE(hints && hints4 && (const void*)hints != (const void*)hints4);
  DCA_REQUIRE(B > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31) && Hc % 4 == 0 && Wc % 4 == 0);
  DCA_REQUIRE(dca_window_ok(Hc, Wc, dst_y0, rows, cols) && dca_window_ok(h, w, src_y0, rows, cols));
  DCA_REQUIRE(maxdisp > 0.f);                                      // (false for a NaN)
  const int H4 = Hc / 4, W4 = Wc / 4;
  const long total = (long)B * H4 * W4;
  hipLaunchKernelGGL(hints_quarter_kernel, dim3(gd_blocks(total)), dim3(GD_THREADS), 0, stream, hints, hints4, B, h, w, H4, W4,
                     src_y0, dst_y0, rows, cols, maxdisp);
  int rc = dca_launch_status();
  if (rc != 0 || count == nullptr) return rc;
  hipLaunchKernelGGL(hints_count_kernel, dim3(1), dim3(GD_THREADS), 0, stream, (const float*)hints4, total, count);
  return dca_launch_status();
}

extern "C" int dca_volume_modulate(const float* in, const float* hints4, float* out, int B, int C, int D, int H, int W, float k,
                                   float i2c2, hipStream_t stream) {
  DCA_REQUIRE(in && hints4 && out && (const void*)hints4 != (const void*)out);
  DCA_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0);
  DCA_REQUIRE(k > 0.f && i2c2 > 0.f && k < INFINITY && i2c2 < INFINITY);
  const bool vec = W % 4 == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)hints4) & 15) == 0;
  const long total = (long)B * D * H * (vec ? W / 4 : W);
  if (vec)
    hipLaunchKernelGGL(modulate_kernel<true>, dim3(gd_blocks(total)), dim3(GD_THREADS), 0, stream, in, hints4, out, B, C, D, H, W,
                       k, i2c2);
  else
    hipLaunchKernelGGL(modulate_kernel<false>, dim3(gd_blocks(total)), dim3(GD_THREADS), 0, stream, in, hints4, out, B, C, D, H, W,
                       k, i2c2);
  return dca_launch_status();
}
