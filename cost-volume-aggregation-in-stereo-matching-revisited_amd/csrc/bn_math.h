// The per-element arithmetic of the BatchNorm kernels (pointwise.hip) for the kernels elsewhere that run a BatchNorm pass
// of their own (conv3d_c1.hip: the logit heads' backward-data folded into the BatchNorm backward).  One definition each:
// two kernels that form the same quantity round alike.
#pragma once
#include "dca_frag.h"

// scale*y + shift of every apply and backward kernel: ONE rounding, written as an explicit fma so that no two kernels (and
// no two forms of one kernel) can contract it differently.
__device__ __forceinline__ float bn_affine(float y, float sc, float sh) { return __fmaf_rn(y, sc, sh); }
// One element's terms of the backward sums (sum g, sum g*xhat).  Not contracted: every reduction over the same (g, y, stats)
// -- bn_bwd_reduce_kernel's own pair and the second pair it forms for a folded skip BatchNorm -- rounds alike.
__device__ __forceinline__ void bn_bwd_acc(float g, float y, float mean, float invstd, float& a0, float& a1) {
#pragma clang fp contract(off)
  a0 += g;
  a1 += g * (y - mean) * invstd;
}

// the two f16 terms of the f16x2 kernels (x2_split) as 16-bit patterns
__device__ __forceinline__ void px2_split(float v, int e, unsigned short& h, unsigned short& l) {
  _Float16 hh, ll;
  x2_split(v, e, hh, ll);
  h = __builtin_bit_cast(unsigned short, hh);
  l = __builtin_bit_cast(unsigned short, ll);
}
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// the chunks of S per channel that bn_bwd_reduce_kernel (pointwise.hip) sums on its own, and their length
void dca_internal_bn_chunking(long S, int C, int* nchunk, long* chunk_len);
// bn_bwd_finalize_kernel (pointwise.hip) for a reduce pass launched elsewhere: nchunk partials per channel in part and, with
// dyexps, as many slots per channel in gmax
int dca_internal_bn_bwd_finalize(const double* part, int nchunk, double count, float* dgb, int C, const float* stats,
                                 int training, const unsigned* gmax, const unsigned* ymax, int ymax_slots, int* dyexps,
                                 hipStream_t stream);
