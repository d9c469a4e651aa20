// Backward of a 1x1x1 convolution with the BatchNorm (+ activation) behind it as ONE pass over memory (gfx950).
//
//   y = conv1x1x1(x [, x2]; W)        z = act(BN(y))        (convbn_3d with kernel 1: `fuse` / `redir` of
//   models/augment/cva.py:16-55, the q/k/v/out projections of models/augment/SelfAttention_bn.py)
//
// Given dz, the kernel forms the gradient of y in registers, with the expression and operation order of
// bn_bwd_apply_kernel's vector path (pointwise.hip) so that it is the tensor that kernel would have written,
//   u = y*sc + sh;  g = dz * (u > 0 ? 1 : slope);  dy = (g - k1 - (y - mean)*k2) * sc,
// and contracts it twice while it sits in LDS:
//   dW[co][ci]  = sum_{n,v} dy[co][v] x[ci][v]      the contraction of wgrad1_kernel<false> (conv3d_wgrad.hip): same tile
//                                                   of 256 voxels, same tile-to-workgroup assignment, same slab format
//                                                   and wgrad_reduce_kernel, hence the same bits;
//   dx[ci][v]   = sum_co W[co][ci] dy[co][v]        the bf16x3 product of conv1_x3_kernel (conv1_x3.hip), term for term:
//                                                   dy's 16-channel chunks are read from the LDS image (lanes along the
//                                                   voxels: conflict free), split into three bf16 terms in registers and
//                                                   multiplied with the same A fragments (built once per workgroup in LDS)
//                                                   in the same order -- the bits of the backward-data launch it replaces;
//                                                   stored as 128-byte row segments per channel.
// dy is never written: per tile the kernel reads dz, y, x (and x2) and writes dx (and dx2) -- 4 (6) passes over a
// 32-channel tensor where reduce-then-apply, backward-data and weight gradient took 7 (11).
// Two inputs (x2 != null, the implicit channel concat of `fuse`): one workgroup, two accumulators; x2's tile replaces x's
// in LDS after the first contraction, so dz and y are read once.
#include "dca_frag.h"
#include "../../include/dca_hip.h"

struct C1bArgs {
  const float *dz, *y, *stats, *dgb, *x, *x2, *w;
  float *part, *dx, *dx2;
  int N, S, ntile, training;
  float slope;
};

template <bool TWO>
__global__ __launch_bounds__(256, 2) void conv1_bwd_fused_kernel(C1bArgs a) {
  constexpr int NV = 256, P = NV + 1, C = 32, CIN = TWO ? 64 : 32, WFRAG = 2 * 3 * 64 * 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;
  float* ys = smem + C * P;
  float* cst = smem + 2 * C * P;   // [mean | sc | sh | k1 | k2][32]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int S = a.S, tiles_per_n = (S + NV - 1) / NV, ntile = a.ntile;
  if (tid < C) {
    const float invstd = a.stats[C + tid];
    cst[tid] = a.stats[tid];
    cst[C + tid] = a.stats[2 * C + tid];
    cst[2 * C + tid] = a.stats[3 * C + tid];
    cst[3 * C + tid] = a.training ? dca_coherent_loadf(a.dgb + 2 * C + tid) : 0.f;
    cst[4 * C + tid] = a.training ? dca_coherent_loadf(a.dgb + 3 * C + tid) * invstd : 0.f;
  }
  // bf16x3 A fragments of W^T, [input][chunk 2][term 3][lane 64][8]: W[b = ci][a = co] = w[co * CIN + 32 * input + ci]
  unsigned short* wl = (unsigned short*)(cst + 5 * C);
  for (int i = tid; i < (TWO ? 2 : 1) * WFRAG; i += 256) wl[i] = w1x3_elem(a.w, i % WFRAG, C, C, 1, CIN, C * (i / WFRAG));
  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.f;

  // dz, y, x, x2 are all (N, 32, S): one byte offset serves the four descriptors
  const long bytes = (long)a.N * C * S * 4;
  const __amdgpu_buffer_rsrc_t dzr = dca_rsrc(a.dz, bytes), yr = dca_rsrc(a.y, bytes), xr = dca_rsrc(a.x, bytes);
  const __amdgpu_buffer_rsrc_t x2r = dca_rsrc(TWO ? a.x2 : a.x, bytes);
  float4 rd[8], ry[8], rx[8], rx2[TWO ? 8 : 1];
  auto load_main = [&](int tile) __attribute__((always_inline)) {
    const int n = tile / tiles_per_n, v0 = (tile % tiles_per_n) * NV;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int v = v0 + 4 * (tid & 63), c = wv + 4 * k, ok = (int)(v < S);
      const int off = ((n * C + c) * S + v) * 4;
      rd[k] = dca_bload4(dzr, off, ok);
      ry[k] = dca_bload4(yr, off, ok);
      rx[k] = dca_bload4(xr, off, ok);
    }
  };
  auto load_x2 = [&](int tile) __attribute__((always_inline)) {
    const int n = tile / tiles_per_n, v0 = (tile % tiles_per_n) * NV;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int v = v0 + 4 * (tid & 63), c = wv + 4 * k, ok = (int)(v < S);
      rx2[k] = dca_bload4(x2r, ((n * C + c) * S + v) * 4, ok);
    }
  };
  if ((int)blockIdx.x < ntile) {
    load_main(blockIdx.x);
    if constexpr (TWO) load_x2(blockIdx.x);
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int n = tile / tiles_per_n, v0 = (tile % tiles_per_n) * NV;
    const int next = tile + (int)gridDim.x;
    __syncthreads();
    {
      const int q = tid & 63;
      const bool ok = v0 + 4 * q < S;     // voxels past the sample's end: x is 0 there, dy must be too
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = wv + 4 * k;
        const float mean = cst[c], sc = cst[C + c], sh = cst[2 * C + c], k1 = cst[3 * C + c], k2 = cst[4 * C + c];
        const float yv[4] = {ry[k].x, ry[k].y, ry[k].z, ry[k].w}, dv[4] = {rd[k].x, rd[k].y, rd[k].z, rd[k].w};
        float* px = xs + c * P + 4 * q;
        float* py = ys + c * P + 4 * q;
        px[0] = rx[k].x; px[1] = rx[k].y; px[2] = rx[k].z; px[3] = rx[k].w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float u = yv[j] * sc + sh;
          const float g = dv[j] * (u > 0.f ? 1.f : a.slope);
          const float o = (g - k1 - (yv[j] - mean) * k2) * sc;
          py[j] = ok ? o : 0.f;
        }
      }
    }
    __syncthreads();
    if (next < ntile) load_main(next);
    const float* xr_ = xs + l31 * P + wv * 64 + half;
    const float* yr_ = ys + l31 * P + wv * 64 + half;
#pragma unroll 8
    for (int p = 0; p < 32; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yr_[2 * p], xr_[2 * p], acc, 0, 0, 0);
    // ---- backward-data for the wave's 64 voxels, 32 per accumulator: conv1_x3_kernel's chunk loop with B from the dy image
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      const float* yb = ys + 8 * half * P + wv * 64 + jb * 32 + l31;
      const int v = v0 + wv * 64 + jb * 32 + l31;
      bf16x8 bh[2], bm[2], bl[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 H, M, L;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float va = yb[(16 * c + 2 * j) * P], vb = yb[(16 * c + 2 * j + 1) * P];
          const unsigned h2 = lp_pack2<__bf16>(va, vb);
          const float ra = va - __uint_as_float(h2 << 16), rb = vb - __uint_as_float(h2 & 0xffff0000u);      // exact
          const unsigned m2 = lp_pack2<__bf16>(ra, rb);
          const unsigned l2 = lp_pack2<__bf16>(ra - __uint_as_float(m2 << 16), rb - __uint_as_float(m2 & 0xffff0000u));
          H[j] = h2; M[j] = m2; L[j] = l2;
        }
        bh[c] = __builtin_bit_cast(bf16x8, H); bm[c] = __builtin_bit_cast(bf16x8, M); bl[c] = __builtin_bit_cast(bf16x8, L);
      }
#pragma unroll
      for (int s = 0; s < (TWO ? 2 : 1); ++s) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const unsigned short* wf = wl + s * WFRAG + (c * 3 * 64 + lane) * 8;
          const bf16x8 w0 = *(const bf16x8*)wf, w1 = *(const bf16x8*)(wf + 512), w2 = *(const bf16x8*)(wf + 1024);
          // smallest terms first, the order of conv1_x3_kernel
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, bl[c], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, bh[c], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, bm[c], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, bm[c], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, bh[c], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, bh[c], d, 0, 0, 0);
        }
        if (v < S) {
          float* o = (s ? a.dx2 : a.dx) + ((long)n * C + 4 * half) * S + v;
#pragma unroll
          for (int r = 0; r < 16; ++r) o[(long)((r & 3) + 8 * (r >> 2)) * S] = d[r] + 0.f;   // + 0: that kernel's epilogue (-0 -> +0)
        }
      }
    }
    if constexpr (TWO) {
      __syncthreads();      // every wave is done with x's image
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float* px = xs + (wv + 4 * k) * P + 4 * (tid & 63);
        px[0] = rx2[k].x; px[1] = rx2[k].y; px[2] = rx2[k].z; px[3] = rx2[k].w;
      }
      __syncthreads();
      if (next < ntile) load_x2(next);
#pragma unroll 8
      for (int p = 0; p < 32; ++p) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(yr_[2 * p], xr_[2 * p], acc2, 0, 0, 0);
    }
  }
  // reduce the 4 waves through LDS, then one slab per workgroup and input (the slab format of wgrad1_kernel)
  float* red = smem;  // [4][1024]
#pragma unroll
  for (int s = 0; s < (TWO ? 2 : 1); ++s) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r)
      red[wv * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + l31] = s ? acc2[r] : acc[r];
    __syncthreads();
    float* part = a.part + ((long)s * gridDim.x + blockIdx.x) * 1024;
    for (int i = tid; i < 1024; i += 256) part[i] = (red[i] + red[1024 + i]) + (red[2048 + i] + red[3072 + i]);
  }
}

// the tile-to-workgroup assignment is the 1x1x1 weight gradient's own (one slab of 1024 floats per workgroup)
static int c1b_workgroups(int N, long S) { return (int)(dca_conv3d_wgrad_workspace(N, 32, 32, 1, 1, (int)S, 1, 1) / 1024); }

extern "C" long dca_conv1_bwd_fused_workspace(int N, long S, int two) {
  if (N <= 0 || S <= 0 || (long)N * 32 * S * 4 >= 0x7ffff000L) return 0;
  return (long)c1b_workgroups(N, S) * 1024 * (two ? 2 : 1);
}

extern "C" int dca_conv1_bwd_fused(const float* dz, const float* y, const float* stats, const float* dgb, float slope,
                                   int training, const float* x, const float* x2, const float* w, float* part, float* dx,
                                   float* dx2, float* dw, long s_cy, long s_cx, int N, int C1, int C2, int Cout, long S,
                                   hipStream_t stream) {
  DCA_REQUIRE(dz && y && stats && dgb && x && w && part && dx && dw && N > 0 && S > 0);
  DCA_REQUIRE(Cout == 32 && C1 == 32 && (C2 == 0 || C2 == 32) && (x2 != nullptr) == (C2 == 32) && (dx2 != nullptr) == (C2 == 32));
  DCA_REQUIRE(S % 4 == 0 && (long)N * 32 * S * 4 < 0x7ffff000L);   // 32-bit byte offsets, a masked tile's tail included
  DCA_REQUIRE((((uintptr_t)dz | (uintptr_t)y | (uintptr_t)x | (uintptr_t)x2) & 15) == 0);
  C1bArgs a;
  a.dz = dz; a.y = y; a.stats = stats; a.dgb = dgb; a.x = x; a.x2 = x2; a.w = w;
  a.part = part; a.dx = dx; a.dx2 = dx2;
  a.N = N; a.S = (int)S; a.ntile = N * cdiv(S, 256); a.training = training; a.slope = slope;
  const int nblk = c1b_workgroups(N, S);
  const size_t lds = (size_t)(2 * 32 * 257 + 5 * 32) * 4 + (size_t)(C2 ? 2 : 1) * 2 * 3 * 64 * 8 * 2;   // images, constants, A fragments
  const void* fn = C2 ? (const void*)conv1_bwd_fused_kernel<true> : (const void*)conv1_bwd_fused_kernel<false>;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  if (C2) hipLaunchKernelGGL(conv1_bwd_fused_kernel<true>, dim3(nblk), dim3(256), lds, stream, a);
  else hipLaunchKernelGGL(conv1_bwd_fused_kernel<false>, dim3(nblk), dim3(256), lds, stream, a);
  int st = dca_launch_status();
  if (st) return st;
  st = dca_internal_wgrad_reduce(part, dw, nblk, 1, 1, 1, 32, 32, s_cy, s_cx, stream);
  if (st || !C2) return st;
  return dca_internal_wgrad_reduce(part + (long)nblk * 1024, dw + 32 * s_cx, nblk, 1, 1, 1, 32, 32, s_cy, s_cx, stream);
}
