// Per-pixel confidence from the disparity distribution (inference only).  The network's last
// step is a soft-max over the maxdisp/4 disparity bins of every 1/4-res pixel (`logits3`, models/gwcnet_dca_g.py); the
// reference reduces it to its mean (the soft-argmin) and drops it.  Three bandwidth-bound kernels keep more of it:
//
//  * soft-argmin statistics -- one thread per (b, pixel), coalesced over HW like softargmin_fwd_kernel (volume.hip):
//    the soft-argmin itself (the SAME helper, so bitwise the same number), the soft-argmin and the probability mass of
//    the window around the arg-max, the normalised entropy and the standard deviation.  The K logits are read once from
//    memory and twice more from cache (maximum + arg-max, moments, window / entropy / variance); two expf per logit.
//  * convex x4 up-sampling of P planes through ONE read of the 144 mask logits -- the soft-max over a sub-pixel's 9
//    neighbours is computed once and applied to every plane (same helpers as convex_up4_fwd_kernel, heads2d.hip, so a
//    plane with scale 4 is bitwise that kernel's result).  Neighbours outside the map are 0 for every plane (F.unfold
//    zero padding): a confidence plane falls at the frame border exactly where the disparity is pulled towards 0.
//  * risk-coverage histogram -- pixels binned by confidence; per bin the count, the sum of |pred - gt| in 2^-20 fixed
//    point and the count of errors > 3, in an LDS histogram per workgroup flushed with 64-bit integer atomics (as
//    region_confusion_kernel, eval_metrics.hip): integer sums are order-free, so the state is bitwise reproducible.
#include "dca_common.h"
#include "dca_softmax.h"
#include "../../include/dca_hip.h"

namespace {

#define CONF_THREADS 256

// ---- (a) soft-argmin statistics ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CONF_THREADS) void softargmin_stats_kernel(const float* __restrict__ x,
                                                                        float* __restrict__ out, int B, int K, long HW,
                                                                        int radius) {
  const long total = (long)B * HW;
  const float logk = logf((float)K);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / HW, p = idx % HW;
    const float* xp = x + b * K * HW + p;
    float m = -INFINITY, s, sk;
    int kstar = 0;                                           // lowest index of the maximum: exact, taken on the logits
    for (int k = 0; k < K; ++k) {                            // m as softmax_moments computes it, with the arg-max beside it
      const float v = xp[k * HW];
      kstar = v > m ? k : kstar;
      m = fmaxf(m, v);
    }
    softmax_sums(xp, K, HW, m, s, sk);
    const float d = sk / s;                                  // == softargmin_fwd_kernel, mode 1
    const int lo = kstar - radius, hi = kstar + radius;      // radius <= K here; the range check clips the window
    float ws = 0.f, wsk = 0.f, et = 0.f, var = 0.f;
    for (int k = 0; k < K; ++k) {
      const float t = xp[k * HW] - m, e = expf(t), dk = (float)k - d;
      const bool in = k >= lo && k <= hi;
      ws += in ? e : 0.f;
      wsk += in ? e * (float)k : 0.f;
      et += e > 0.f ? e * t : 0.f;                           // an underflowed e_k contributes 0 (no 0 * inf)
      var += e * dk * dk;
    }
    float* op = out + b * DCA_CONF_PLANES * HW + p;
    op[DCA_CONF_DISP * HW] = d;
    op[DCA_CONF_DUNI * HW] = wsk / ws;
    op[DCA_CONF_MASS * HW] = ws / s;
    op[DCA_CONF_ENT * HW] = K > 1 ? (logf(s) - et / s) / logk : 0.f;     // a uniform distribution gives exactly 1
    op[DCA_CONF_STD * HW] = sqrtf(var / s);
  }
}

// ---- (b) convex x4 up-sampling of P planes ----------------------------------------------------------------------------------
struct PlaneScales { float v[DCA_CONF_MAX_PLANES]; };

template <int P>
__global__ __launch_bounds__(CONF_THREADS) void convex_up4_planes_kernel(const float* __restrict__ logits,
                                                                         const float* __restrict__ planes,
                                                                         PlaneScales scales, float* __restrict__ up,
                                                                         int h, int w) {
  const int b = blockIdx.y, cell = blockIdx.x * CONF_THREADS + threadIdx.x, hw = h * w;
  if (cell >= hw) return;
  const int y = cell / w, x = cell - y * w;
  float nb[P][9];
#pragma unroll
  for (int p = 0; p < P; ++p) convex_load_nb(planes + ((long)b * P + p) * hw, h, w, y, x, scales.v[p], nb[p]);
  const float* lg = logits + (long)b * 144 * hw + cell;
  float* o = up + (long)b * P * 16 * hw + (long)(4 * y) * (4 * w) + 4 * x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float r[P][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e[9];
      const float s = convex_weights(lg, hw, i * 4 + j, e);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc += e[k] * nb[p][k];
        r[p][j] = acc / s;
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
      *(float4*)(o + (long)p * 16 * hw + (long)i * (4 * w)) = make_float4(r[p][0], r[p][1], r[p][2], r[p][3]);
  }
}

template <int P>
int convex_up4_planes_launch(const float* mask_logits, const float* planes, const PlaneScales& sc, float* up, int B,
                             int h, int w, hipStream_t stream) {
  hipLaunchKernelGGL(convex_up4_planes_kernel<P>, dim3(cdiv((long)h * w, CONF_THREADS), B), dim3(CONF_THREADS), 0, stream,
                     mask_logits, planes, sc, up, h, w);
  return dca_launch_status();
}

// ---- (c) risk-coverage histogram ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(CONF_THREADS) void conf_histogram_kernel(const float* __restrict__ conf,
                                                                      const float* __restrict__ pred,
                                                                      const float* __restrict__ gt,
                                                                      unsigned long long* __restrict__ state, long total,
                                                                      int nbins, float maxdisp) {
  extern __shared__ unsigned long long hist[];     // nbins * 3
  for (int i = threadIdx.x; i < nbins * 3; i += CONF_THREADS) hist[i] = 0;
  __syncthreads();
  for (long idx = (long)blockIdx.x * CONF_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * CONF_THREADS) {
    const float c = conf[idx], g = gt[idx];
    if (g > 0.f && g < maxdisp && c == c) {
      const int raw = (int)(fminf(fmaxf(c, 0.f), 1.f) * (float)nbins);
      const int bin = raw < nbins - 1 ? raw : nbins - 1;
      const float err = fabsf(pred[idx] - g);
      atomicAdd(&hist[bin * 3 + 0], 1ull);
      atomicAdd(&hist[bin * 3 + 1], (unsigned long long)(long long)(err * 1048576.f));   // exact scaling, truncated
      if (err > 3.f) atomicAdd(&hist[bin * 3 + 2], 1ull);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins * 3; i += CONF_THREADS) {
    const unsigned long long n = hist[i];
    if (n) atomicAdd(&state[i], n);
  }
}

}  // namespace

extern "C" int dca_softargmin_stats(const float* logits, float* out, int B, int K, long HW, int radius,
                                    hipStream_t stream) {
  DCA_REQUIRE(logits && out && B > 0 && K >= 1 && HW > 0 && radius >= 0);
  const long total = (long)B * HW, g = (total + CONF_THREADS - 1) / CONF_THREADS;
  hipLaunchKernelGGL(softargmin_stats_kernel, dim3((int)(g < 4096 ? g : 4096)), dim3(CONF_THREADS), 0, stream, logits, out,
                     B, K, HW, radius < K ? radius : K);
  return dca_launch_status();
}

extern "C" int dca_convex_up4_planes(const float* mask_logits, const float* planes, const float* scales, float* up, int B,
                                     int P, int h, int w, hipStream_t stream) {
  DCA_REQUIRE(mask_logits && planes && scales && up && P >= 1 && P <= DCA_CONF_MAX_PLANES);
  DCA_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && (long)h * w < (1L << 31) / 16);
  DCA_REQUIRE((((uintptr_t)up) & 15) == 0);
  PlaneScales sc;
  for (int p = 0; p < DCA_CONF_MAX_PLANES; ++p) sc.v[p] = p < P ? scales[p] : 0.f;
  switch (P) {
    case 1: return convex_up4_planes_launch<1>(mask_logits, planes, sc, up, B, h, w, stream);
    case 2: return convex_up4_planes_launch<2>(mask_logits, planes, sc, up, B, h, w, stream);
    case 3: return convex_up4_planes_launch<3>(mask_logits, planes, sc, up, B, h, w, stream);
    case 4: return convex_up4_planes_launch<4>(mask_logits, planes, sc, up, B, h, w, stream);
    case 5: return convex_up4_planes_launch<5>(mask_logits, planes, sc, up, B, h, w, stream);
    case 6: return convex_up4_planes_launch<6>(mask_logits, planes, sc, up, B, h, w, stream);
    case 7: return convex_up4_planes_launch<7>(mask_logits, planes, sc, up, B, h, w, stream);
    default: return convex_up4_planes_launch<8>(mask_logits, planes, sc, up, B, h, w, stream);
  }
}

extern "C" int dca_conf_histogram(const float* conf, const float* pred, const float* gt, long long* state, int B, long HW,
                                  int nbins, float maxdisp, hipStream_t stream) {
  DCA_REQUIRE(conf && pred && gt && state && B > 0 && HW > 0 && nbins >= 2 && nbins <= DCA_CONF_MAX_BINS);
  const long total = (long)B * HW, g = (total + (long)CONF_THREADS * 8 - 1) / ((long)CONF_THREADS * 8);   // >= 8 pixels per thread
  hipLaunchKernelGGL(conf_histogram_kernel, dim3((int)(g < 1024 ? g : 1024)), dim3(CONF_THREADS),
                     (size_t)nbins * 3 * sizeof(unsigned long long), stream, conf, pred, gt, (unsigned long long*)state,
                     total, nbins, maxdisp);
  return dca_launch_status();
}
