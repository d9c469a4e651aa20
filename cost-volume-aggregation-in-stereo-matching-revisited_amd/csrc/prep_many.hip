// One launch that re-lays-out MANY convolution weights (the fp32 wt[tap][cin][cout] images of conv3d_mfma.hip and the
// pre-split bf16x3 fragment images of conv3d_bf16x3.hip / conv1_x3.hip, laid out by the element functions of dca_frag.h): a
// training step re-packs every weight twice (forward and backward-data layouts) right after the optimizer update, which as
// ~130 separate 5-us launches costs more GPU time than the work itself.  The descriptors live in a device table built once (ops.PrepackPlan).
#include "dca_frag.h"

namespace {

struct PrepDesc {          // mirrored by ops.PrepackPlan (72 bytes)
  const float* src;
  void* dst;
  int kind;                // 0: fp32 image (dca_conv3d_prep_weight), 1: bf16x3 image (dca_conv3d_x3_prep_weight),
                           // 2: bf16x3 fragments of a 1x1x1 conv (dca_conv1_x3_prep_weight)
                           // (the f16x2 images of dca_conv3d_x2_prep_weight depend on the operand's per-channel exponents and
                           // are packed per launch: not part of a plan)
  int A, Bn, Apad, Bpad, K, src_ab, flip, Btotal, b_off, NCH, pad_;
  long total;              // elements of dst
};

__global__ __launch_bounds__(256) void prep_many_kernel(const PrepDesc* __restrict__ table) {
  const PrepDesc d = table[blockIdx.y];
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < d.total; idx += (long)gridDim.x * 256) {
    if (d.kind == 0) ((float*)d.dst)[idx] = wt_f32_elem(d.src, idx, d.A, d.Bn, d.Apad, d.Bpad, d.K, d.src_ab, d.flip, d.Btotal, d.b_off);
    else if (d.kind == 2) ((unsigned short*)d.dst)[idx] = w1x3_elem(d.src, idx, d.A, d.Bn, d.src_ab, d.Btotal, d.b_off);
    else if (d.kind == 1) ((unsigned short*)d.dst)[idx] = wx3_elem(d.src, idx, d.A, d.Bn, d.NCH, d.src_ab, d.flip);
  }
}

}  // namespace

// table: n device-resident 72-byte descriptors {src, dst, kind, A, Bn, Apad, Bpad, K, src_ab, flip, Btotal, b_off, NCH,
// pad, total} (pointers 8 bytes, ints 4, total 8) with the argument meaning of dca_conv3d_prep_weight (kind 0) /
// dca_conv3d_x3_prep_weight (kind 1: A, Bn, src_ab, flip, NCH = ceil(A/16), total = weight_bytes/2) /
// dca_conv1_x3_prep_weight (kind 2: A, Bn, src_ab, Btotal, b_off, total = weight_bytes/2).
extern "C" int dca_conv3d_prep_many(const void* table, int n, hipStream_t stream) {
  DCA_REQUIRE(table && n > 0 && n <= 65535 && (((uintptr_t)table) & 7) == 0);
  hipLaunchKernelGGL(prep_many_kernel, dim3(48, n), dim3(256), 0, stream, (const PrepDesc*)table);
  return dca_launch_status();
}
