// Guided stereo: the factor a sparse disparity hint puts on the cost volume.  ONE definition, called
// by the fused builder (volume_fused.hip) and by the stand-alone pass (guided.hip): the two routes produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

// m(d, h4) of include/dca_hip.h: k exp(-(d - h4)^2 / (2 c^2)) at a cell with a hint (h4 > 0), exactly 1 elsewhere (a NaN is
// no hint).  Every product is rounded on its own, so no call site can contract it differently.
__device__ __forceinline__ float dca_guide_factor(int d, float h4, float k, float inv2c2) {
  const float t = (float)d - h4;
  const float e = __fmul_rn(__fmul_rn(t, t), inv2c2);
  return h4 > 0.f ? __fmul_rn(k, expf(-e)) : 1.0f;
}
