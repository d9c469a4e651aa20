// The two soft-max cores that more than one kernel needs, ONE copy each, so that kernels which promise bitwise equal
// results (soft-argmin and plane 0 of the soft-argmin statistics; the convex up-sampler for one plane and for several)
// run the same operations in the same order.
#pragma once
#include "dca_common.h"

// The K logits of one pixel, xp[k * HW], and their maximum m (fmaxf over ascending k from -INFINITY):  s = sum_k e_k,
// sk = sum_k k e_k  with e_k = expf(x_k - m), summed in ascending k.  sk / s is the soft-argmin.
__device__ __forceinline__ void softmax_sums(const float* __restrict__ xp, int K, long HW, float m, float& s, float& sk) {
  s = 0.f;
  sk = 0.f;
  for (int k = 0; k < K; ++k) {
    const float e = expf(xp[k * HW] - m);
    s += e;
    sk += e * (float)k;
  }
}
// the maximum, then the sums
__device__ __forceinline__ void softmax_moments(const float* __restrict__ xp, int K, long HW, float& m, float& s,
                                                float& sk) {
  m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, xp[k * HW]);
  softmax_sums(xp, K, HW, m, s, sk);
}

// Convex x4 up-sampling (heads2d.hip): the 3x3 neighbourhood of cell (y, x) of the 1/4-res map d (h, w), times `scale`;
// neighbours outside the map are 0 (F.unfold zero padding of scale * d).
__device__ __forceinline__ void convex_load_nb(const float* __restrict__ d, int h, int w, int y, int x, float scale,
                                               float (&nb)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    const bool ok = (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w;
    nb[k] = ok ? scale * d[(long)yy * w + xx] : 0.f;
  }
}

// Un-normalised soft-max weights of sub-pixel ij = i * 4 + j of a cell over its 9 neighbours: lg points at the cell's
// first mask logit (channel = k * 16 + ij, channel stride hw).  e[k] = expf(v_k - max_k v); returns sum_k e[k].
// An up-sampled value is (sum_k e[k] * nb[k]) / sum, accumulated in ascending k.
__device__ __forceinline__ float convex_weights(const float* __restrict__ lg, long hw, int ij, float (&e)[9]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = lg[(long)(k * 16 + ij) * hw];
    m = fmaxf(m, e[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = expf(e[k] - m);
    s += e[k];
  }
  return s;
}
