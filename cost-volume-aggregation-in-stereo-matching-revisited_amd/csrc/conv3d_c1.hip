// 3x3x3 convolution with ONE output channel (the logit heads), gfx950.
//
// Replaces nn.Conv3d(32, 1, kernel_size=3, padding=1, bias=False): `classif{0..3}.2`
// (models/gwcnet_dca_g.py:154-168) and `cva.classify.2` (models/augment/cva.py:51-53), forward, backward-data and
// weight gradient.  With a single output channel a direct MFMA tile would waste 31 of its 32 rows; instead the 27
// taps become the GEMM's output axis (see "tap expansion" below) for forward and weight gradient, and the
// backward-data pass is a VALU kernel (dy halo tile in LDS, 4 consecutive W positions per thread).
#include "dca_common.h"
#include "dca_tiles.h"
#include "bn_math.h"
#include "../../include/dca_hip.h"

namespace {
constexpr int TD = 4, TH = 8, TW = 32, CK = 4;
constexpr int ID = TD + 2, IH = TH + 2, IWP = 40;

struct C1Args {
  const float* x;   // (N, C, D, H, W)
  const float* w;   // (1, C, 3, 3, 3)
  const float* dy;  // (N, 1, D, H, W)
  float* out;       // fwd: y (N,1,..); bwd-data: dx (N,C,..); wgrad: part [nblk][C][27]
  int N, C, D, H, W;
  int nTD, nTH, nTW, ntiles;
  int vec;
};

// stage `nch` channel planes (starting at channel c0 of sample n, C channels per sample) of a halo tile into LDS
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, float* lds, int n, int C, int c0, int nch,
                                           int D, int H, int W, int d0, int h0, int w0, int vec, int tid) {
  const int rows = nch * ID * IH;
  if (vec) {
    for (int it = tid; it < rows * 8; it += 256) {
      const int row = it >> 3, q = it & 7;
      const int c = row / (ID * IH), rem = row % (ID * IH), id = rem / IH, ih = rem % IH;
      const int ci = c0 + c, d = d0 - 1 + id, h = h0 - 1 + ih, wq = w0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ci < C && (unsigned)d < (unsigned)D && (unsigned)h < (unsigned)H && wq < W)
        v = *(const float4*)(src + ((((long)n * C + ci) * D + d) * H + h) * W + wq);
      *(float4*)(lds + row * IWP + 4 + 4 * q) = v;
    }
    for (int it = tid; it < rows * 2; it += 256) {
      const int row = it >> 1, j = (it & 1) ? 33 : 0;
      const int c = row / (ID * IH), rem = row % (ID * IH), id = rem / IH, ih = rem % IH;
      const int ci = c0 + c, d = d0 - 1 + id, h = h0 - 1 + ih, wi = w0 - 1 + j;
      float v = 0.f;
      if (ci < C && (unsigned)d < (unsigned)D && (unsigned)h < (unsigned)H && (unsigned)wi < (unsigned)W)
        v = src[((((long)n * C + ci) * D + d) * H + h) * W + wi];
      lds[row * IWP + 3 + j] = v;
    }
  } else {
    for (int it = tid; it < rows * 34; it += 256) {
      const int row = it / 34, j = it % 34;
      const int c = row / (ID * IH), rem = row % (ID * IH), id = rem / IH, ih = rem % IH;
      const int ci = c0 + c, d = d0 - 1 + id, h = h0 - 1 + ih, wi = w0 - 1 + j;
      float v = 0.f;
      if (ci < C && (unsigned)d < (unsigned)D && (unsigned)h < (unsigned)H && (unsigned)wi < (unsigned)W)
        v = src[((((long)n * C + ci) * D + d) * H + h) * W + wi];
      lds[row * IWP + 3 + j] = v;
    }
  }
}

__device__ __forceinline__ void tile_coords(const C1Args& a, int tile, int& n, int& d0, int& h0, int& w0) {
  dca_tile_decode<TD, TH, TW>(tile, a.nTD, a.nTH, a.nTW, n, d0, h0, w0);
}

// ------------------------------------------------------------------------------------------ backward-data
// dx[n,ci,v] = sum_k dy[n,0,v+1-k] w[ci][k] = sum_t dy[v+t-1] w[ci][26-t]
// the weights as the backward-data kernels read them from LDS: [C][9][4], flipped
__device__ __forceinline__ void c1_stage_weights(const float* __restrict__ w, float* w_lds, int C, int tid) {
  for (int i = tid; i < C * 27; i += 256) {
    const int c = i / 27, t = i % 27;
    w_lds[(c * 9 + t / 3) * 4 + t % 3] = w[c * 27 + 26 - t];
  }
}
// the thread's window of the dy halo tile: 3 x 3 rows (d, h) of 4 + 2 consecutive w
__device__ __forceinline__ void c1_window(const float* dy_lds, int dl, int hl, int wq, float (&g)[9][6]) {
#pragma unroll
  for (int r9 = 0; r9 < 9; ++r9) {
    const float* p = dy_lds + ((dl + r9 / 3) * IH + hl + r9 % 3) * IWP + 4 * wq;
    const float4 v = *(const float4*)(p + 4);
    g[r9][0] = p[3]; g[r9][1] = v.x; g[r9][2] = v.y; g[r9][3] = v.z; g[r9][4] = v.w; g[r9][5] = p[8];
  }
}
// dx of channel c at the thread's 4 voxels: ONE statement of the order of the 27 products for every kernel that forms it
__device__ __forceinline__ void c1_dx4_row(const float (&g)[6], float wx, float wy, float wz, float (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)      // three chained FMAs (the sum-then-add form costs a multiply and an add more per tap row)
    acc[j] = fmaf(wz, g[j + 2], fmaf(wy, g[j + 1], fmaf(wx, g[j], acc[j])));
}
__device__ __forceinline__ void c1_dx4(const float* w_lds, int c, const float (&g)[9][6], float (&acc)[4]) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
#pragma unroll
  for (int r9 = 0; r9 < 9; ++r9) {
    const float4 wv = *(const float4*)(w_lds + (c * 9 + r9) * 4);
    c1_dx4_row(g[r9], wv.x, wv.y, wv.z, acc);
  }
}
// the same from the weight tensor itself, channel c's 27 taps at wc: c is the same in every lane, so these are scalar loads and
// the weights are scalar operands of the FMAs -- no LDS read and no vector register for them (a kernel that keeps y, the BatchNorm
// terms and the window in registers has none to spare: 36 per channel in flight for the LDS form)
__device__ __forceinline__ void c1_dx4_s(const float* __restrict__ wc, const float (&g)[9][6], float (&acc)[4]) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
#pragma unroll
  for (int r9 = 0; r9 < 9; ++r9) c1_dx4_row(g[r9], wc[26 - 3 * r9], wc[25 - 3 * r9], wc[24 - 3 * r9], acc);
}

__global__ __launch_bounds__(256) void c1_bwd_data_kernel(C1Args a) {
  __shared__ __attribute__((aligned(16))) float dy_lds[ID * IH * IWP];
  extern __shared__ __attribute__((aligned(16))) float w_lds[];  // [C][9][4], flipped
  const int tid = threadIdx.x, wq = tid & 7, row = tid >> 3, dl = row >> 3, hl = row & 7;
  int n, d0, h0, w0;
  tile_coords(a, xcd_remap(blockIdx.x, gridDim.x), n, d0, h0, w0);
  stage_tile(a.dy, dy_lds, n, 1, 0, 1, a.D, a.H, a.W, d0, h0, w0, a.vec, tid);
  c1_stage_weights(a.w, w_lds, a.C, tid);
  __syncthreads();
  float g[9][6];
  c1_window(dy_lds, dl, hl, wq, g);
  const int d = d0 + dl, h = h0 + hl, w = w0 + 4 * wq;
  const bool ok = d < a.D && h < a.H && w < a.W;
  for (int c = 0; c < a.C; ++c) {
    float acc[4];
    c1_dx4(w_lds, c, g, acc);
    if (ok) {
      float* o = a.out + ((((long)n * a.C + c) * a.D + d) * a.H + h) * a.W + w;
      if (a.vec) {
        *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (w + j < a.W) o[j] = acc[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ backward-data inside the BatchNorm backward
// The head's input h = relu(BN(y)) has one reader, the head, so its gradient dh = c1_bwd_data(dlogit, w) is needed only by
// the two passes of that BatchNorm's backward (pointwise.hip: bn_bwd_reduce_kernel, bn_bwd_apply_pack_kernel).  Both are
// restated here and form dh in registers from a 9 x 6 window of dlogit (c1_dx4_s: the bits c1_bwd_data_kernel writes) while
// they stream y: dh is neither written nor read, 3 x 4 bytes per element of (N,C,D,H,W) less.  The reduce pass keeps the
// element order of bn_bwd_reduce_kernel, the apply pass walks the tiles of c1_bwd_data_kernel with persistent workgroups; every
// result is bit for bit that of the three launches.  C == BC, W % 4 == 0, 16-byte aligned tensors (the launcher requires it).
constexpr int BC = 32;

// (the head's weight (1, BC, 3, 3, 3) and the packed dy are kernel arguments of their own: __restrict__, so that the weight
// loads stay scalar beside the kernel's stores)
struct C1BnArgs {
  const float* dlogit;  // (N, 1, D, H, W)
  const float* y;      // (N, BC, D, H, W): the BatchNorm's input
  const float* stats;   // [mean | invstd | scale | shift]
  const float* dgb;     // apply: bn_bwd_finalize_kernel's output
  const int* dyexps;    // apply: the same kernel's exponents
  double* part;         // reduce: [BC][nwg][2]
  unsigned* gmax;       // reduce: slots [c][wg]
  int N, D, H, W;
  int nTD, nTH, nTW, ntiles;
  float slope;
  int training;
};

// the thread index as the staging code of a persistent kernel takes it: opaque, so that the index arithmetic of stage_tile is
// redone per tile -- hoisted out of the tile loop its two dozen values sit in registers through the channel loop and spill
__device__ __forceinline__ int c1_per_tile(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

// bn_bwd_reduce_kernel (pointwise.hip) with dz = dh formed here, in THAT kernel's order: the sums are fp32 per lane, so their
// bits are the order of the additions, and the training step's results must not move.  Workgroup (chunk ch, group of RCG
// channels); lane tid takes the elements i = s0 + 4 tid + 1024 k of the chunk, samples descending, exactly the sequence of
// lane tid of that kernel's block (c, ch) for each of its RCG channels, with the same chunking (the launcher takes it from
// pointwise.hip), the same per-element expressions (bn_affine, bn_bwd_acc) and the same reduction over the workgroup: part
// and max |g| are that kernel's bits given the dh that c1_bwd_data_kernel writes, which c1_dx4_s forms.  The 9 x 6 window of
// dlogit comes straight from memory (hardware-predicated loads, zero outside the volume; neighbouring lanes and the channel
// groups share it in the caches) and is paid once per RCG channels.
constexpr int RCG = 4;
__global__ __launch_bounds__(256, 2) void c1_bn_bwd_reduce_kernel(C1BnArgs a, const float* __restrict__ wt, int nchunk,
                                                                  int chunk_len) {
  const int ch = blockIdx.x, cg = blockIdx.y, tid = threadIdx.x;
  const int HW = a.H * a.W, S = a.D * HW;
  const int s0 = ch * chunk_len, s1 = min(S, s0 + chunk_len);
  float mean[RCG], invstd[RCG], sc[RCG], sh[RCG], a0[RCG], a1[RCG], gm[RCG];
#pragma unroll
  for (int j = 0; j < RCG; ++j) {
    const int c = cg * RCG + j;
    mean[j] = a.stats[c]; invstd[j] = a.stats[BC + c]; sc[j] = a.stats[2 * BC + c]; sh[j] = a.stats[3 * BC + c];
    a0[j] = a1[j] = gm[j] = 0.f;
  }
  for (int n = a.N - 1; n >= 0; --n) {
    const __amdgpu_buffer_rsrc_t rd = dca_rsrc(a.dlogit + (long)n * S, (long)S * 4);
    const __amdgpu_buffer_rsrc_t ry = dca_rsrc(a.y + (long)n * BC * S, (long)BC * S * 4);
    for (int i = s0 + 4 * tid; i < s1; i += 1024) {
      const int d = i / HW, r = i - d * HW, h = r / a.W, w = r - h * a.W;      // W % 4 == 0: the 4 elements share a row
      float g[9][6];
#pragma unroll
      for (int r9 = 0; r9 < 9; ++r9) {
        const int dd = d + r9 / 3 - 1, hh = h + r9 % 3 - 1;
        const int okr = (int)((unsigned)dd < (unsigned)a.D) & (int)((unsigned)hh < (unsigned)a.H);
        const int base = ((dd * a.H + hh) * a.W + w) * 4;
        const float4 v = dca_bload4(rd, base, okr);
        g[r9][0] = dca_bload1(rd, base - 4, okr & (int)(w > 0));
        g[r9][1] = v.x; g[r9][2] = v.y; g[r9][3] = v.z; g[r9][4] = v.w;
        g[r9][5] = dca_bload1(rd, base + 16, okr & (int)(w + 4 < a.W));
      }
      float4 yv[RCG];
#pragma unroll
      for (int j = 0; j < RCG; ++j) yv[j] = dca_bload4(ry, ((cg * RCG + j) * S + i) * 4, 1);
#pragma unroll
      for (int j = 0; j < RCG; ++j) {
        float dh[4];
        c1_dx4_s(wt + (cg * RCG + j) * 27, g, dh);
        const float ys[4] = {yv[j].x, yv[j].y, yv[j].z, yv[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float u = bn_affine(ys[e], sc[j], sh[j]);
          const float gg = dh[e] * (u > 0.f ? 1.f : a.slope);
          bn_bwd_acc(gg, ys[e], mean[j], invstd[j], a0[j], a1[j]);
          gm[j] = fmaxf(gm[j], fabsf(gg));
        }
      }
    }
  }
  __shared__ double red[8];
#pragma unroll
  for (int j = 0; j < RCG; ++j) {
    const int c = cg * RCG + j;
    const double d0 = wave_sum_d((double)a0[j]), d1 = wave_sum_d((double)a1[j]);
    __syncthreads();                       // the previous channel's sums have been read
    if ((tid & 63) == 0) { red[(tid >> 6) * 2] = d0; red[(tid >> 6) * 2 + 1] = d1; }
    __syncthreads();
    if (tid == 0) {
      a.part[((long)c * nchunk + ch) * 2 + 0] = red[0] + red[2] + red[4] + red[6];
      a.part[((long)c * nchunk + ch) * 2 + 1] = red[1] + red[3] + red[5] + red[7];
    }
    dca_cmax_put(gm[j], a.gmax + (long)c * DCA_AMAX_CSLOTS + ch);
  }
}


// bn_bwd_apply_pack_kernel with dz = dh formed here (the bits the reduce pass saw): a thread takes its 4 voxels x 8 channels
// per group and stores whole 16-byte words of both terms.  Window, 8 channels of y and the 8 words under way are 118 registers.
// (The f16 terms are paired into 32-bit words as they are formed: as two vectors of 8 halves per voxel they sat in a register
// each until the store, and the kernel spilled.)
__global__ __launch_bounds__(256, 4) void c1_bn_bwd_apply_pack_kernel(C1BnArgs a, const float* __restrict__ wt,
                                                                      char* __restrict__ dyp) {
  __shared__ __attribute__((aligned(16))) float dy_lds[ID * IH * IWP];
  __shared__ __attribute__((aligned(16))) float k_lds[BC * 8];   // mean, scale, shift, k1, k2, exponent (bits), -, -
  const int tid = threadIdx.x, wq = tid & 7, row = tid >> 3, dl = row >> 3, hl = row & 7;
  const int S = a.D * a.H * a.W;
  if (tid < BC) {
    const int c = tid;
    float* k = k_lds + c * 8;
    k[0] = a.stats[c]; k[1] = a.stats[2 * BC + c]; k[2] = a.stats[3 * BC + c];
    k[3] = a.training ? dca_coherent_loadf(a.dgb + 2 * BC + c) : 0.f;
    k[4] = a.training ? dca_coherent_loadf(a.dgb + 3 * BC + c) * a.stats[BC + c] : 0.f;
    k[5] = __int_as_float(dca_coherent_loadi(a.dyexps + c));
  }
  const long tb = px2_term_bytes(BC, S);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += (int)gridDim.x) {
    int n, d0, h0, w0;
    dca_tile_decode<TD, TH, TW>(tile, a.nTD, a.nTH, a.nTW, n, d0, h0, w0);
    __syncthreads();
    stage_tile(a.dlogit, dy_lds, n, 1, 0, 1, a.D, a.H, a.W, d0, h0, w0, 1, c1_per_tile(tid));
    __syncthreads();
    float g[9][6];
    c1_window(dy_lds, dl, hl, wq, g);
    const int d = d0 + dl, h = h0 + hl, w = w0 + 4 * wq;
    const int ok = (int)(d < a.D) & (int)(h < a.H) & (int)(w < a.W);
    const __amdgpu_buffer_rsrc_t ry = dca_rsrc(a.y + (long)n * BC * S, (long)BC * S * 4);
    const int vox = (d * a.H + h) * a.W + w;
    char* ob = dyp + (long)n * 2 * tb + (long)vox * 16;
#pragma unroll 1
    for (int cg = 0; cg < BC / 8; ++cg) {
      float4 yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) yv[j] = dca_bload4(ry, ((cg * 8 + j) * S + vox) * 4, ok);
      unsigned hv[4][4], lv[4][4];             // [voxel][channel pair]: the 16-byte words of the two terms
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cg * 8 + j;
        float dh[4];
        c1_dx4_s(wt + c * 27, g, dh);
        const float4 ka = *(const float4*)(k_lds + c * 8), kb = *(const float4*)(k_lds + c * 8 + 4);
        const float mean = ka.x, sc = ka.y, sh = ka.z, k1 = ka.w, k2 = kb.x;
        const int ex = __float_as_int(kb.y);
        const float ys[4] = {yv[j].x, yv[j].y, yv[j].z, yv[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float u = bn_affine(ys[e], sc, sh);
          const float gg = dh[e] * (u > 0.f ? 1.f : a.slope);
          const float o = (gg - k1 - (ys[e] - mean) * k2) * sc;
          unsigned short hh, ll;
          px2_split(o, ex, hh, ll);
          if (j % 2 == 0) {
            hv[e][j / 2] = hh; lv[e][j / 2] = ll;
          } else {
            hv[e][j / 2] |= (unsigned)hh << 16; lv[e][j / 2] |= (unsigned)ll << 16;
          }
        }
      }
      if (ok) {
        char* p = ob + (long)cg * S * 16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *(uint4*)(p + e * 16) = make_uint4(hv[e][0], hv[e][1], hv[e][2], hv[e][3]);
          *(uint4*)(p + tb + e * 16) = make_uint4(lv[e][0], lv[e][1], lv[e][2], lv[e][3]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ tap expansion
// (A direct fp32 forward kernel -- the mirror image of the backward-data kernel, channels through LDS four at a time -- was
// built and measured in round 3: 0.80 ms per batch-4 head against 0.47 ms for tap GEMM + gather: 27 LDS reads per channel and
// thread; withdrawn.)
// The forward and the weight gradient are expressed as 1x1x1 GEMMs over a 27-channel "tap" axis so they run on
// the matrix-core kernels of conv3d_mfma.hip / conv3d_wgrad.hip:
//   forward : T[t][v'] = sum_ci w[ci][t] x[ci][v']  (conv1_mfma_kernel, 32 -> 27)      y[v] = sum_t T[t][v + t - 1]
//   wgrad   : G[t][v'] = dy[v' - (t - 1)]                                              dW[ci][t] = sum_v' x[ci][v'] G[t][v']
// (t - 1) is the 3D tap offset (kd-1, kh-1, kw-1); out-of-volume positions contribute zero.
// grid (voxel tiles, N): the sample base is wave-uniform, so each of the 27 shifted taps is one hardware-predicated
// buffer load (one descriptor per kd slab of 9 tap planes) -- 27 independent loads in flight, no branches.
__global__ __launch_bounds__(256) void c1_gather_kernel(const float* __restrict__ T, float* __restrict__ y, int D, int H,
                                                        int W) {
  const long DHW = (long)D * H * W;
  const long n = blockIdx.y;
  const float* p = T + n * 27 * DHW;
  const long end = min(DHW, ((long)blockIdx.x + 1) * 1024);
  for (long idx = (long)blockIdx.x * 1024 + threadIdx.x; idx < end; idx += 256) {
    const int w = idx % W;
    const int t = (int)(idx / W);
    const int h = t % H, d = t / H;
    float s = 0.f;
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int dd = d + kd - 1;
      const __amdgpu_buffer_rsrc_t r = dca_rsrc(p + kd * 9 * DHW, 9 * DHW * 4);  // one descriptor per kd slab
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = w + kw - 1;
          const int ok = (int)((unsigned)dd < (unsigned)D) & (int)((unsigned)hh < (unsigned)H) & (int)((unsigned)ww < (unsigned)W);
          s += dca_bload1(r, ((kh * 3 + kw) * (int)DHW + (dd * H + hh) * W + ww) * 4, ok);
        }
      }
    }
    y[n * DHW + idx] = s;
  }
}

// G[n][tap][v] = dy[n][v - offset(tap)] (0 outside): grid (voxel tiles, 27 taps, N), 32-bit index arithmetic only
// (the former flat version spent its time in 64-bit div/mod chains: 135 us for a 170 MB store stream).
__global__ __launch_bounds__(256) void c1_expand_kernel(const float* __restrict__ dy, float* __restrict__ G, int D, int H,
                                                        int W) {
  const int DHW = D * H * W, tap = blockIdx.y;
  const long n = blockIdx.z;
  const int od = tap / 9 - 1, oh = (tap / 3) % 3 - 1, ow = tap % 3 - 1;
  const __amdgpu_buffer_rsrc_t dr = dca_rsrc(dy + n * DHW, (long)DHW * 4);
  float* out = G + (n * 27 + tap) * (long)DHW;
  const int end = min(DHW, ((int)blockIdx.x + 1) * 1024);
  for (int idx = blockIdx.x * 1024 + threadIdx.x; idx < end; idx += 256) {
    const int w = idx % W, t = idx / W, h = t % H, d = t / H;
    const int dd = d - od, hh = h - oh, ww = w - ow;
    const int ok = (int)((unsigned)dd < (unsigned)D) & (int)((unsigned)hh < (unsigned)H) & (int)((unsigned)ww < (unsigned)W);
    out[idx] = dca_bload1(dr, ((dd * H + hh) * W + ww) * 4, ok);
  }
}

// the same with four consecutive w per thread and one 16-byte store (W % 4 == 0, 16-byte aligned G): the scalar form wrote its
// 680 MB (batch 4, 48x136x240) at 2.6 TB/s
__global__ __launch_bounds__(256) void c1_expand4_kernel(const float* __restrict__ dy, float* __restrict__ G, int D, int H,
                                                         int W) {
  const int DHW = D * H * W, Q = DHW >> 2, WQ = W >> 2, tap = blockIdx.y;
  const long n = blockIdx.z;
  const int od = tap / 9 - 1, oh = (tap / 3) % 3 - 1, ow = tap % 3 - 1;
  const __amdgpu_buffer_rsrc_t dr = dca_rsrc(dy + n * DHW, (long)DHW * 4);
  float* out = G + (n * 27 + tap) * (long)DHW;
  const int end = min(Q, ((int)blockIdx.x + 1) * 1024);
  for (int q = blockIdx.x * 1024 + threadIdx.x; q < end; q += 256) {
    const int wq = q % WQ, t = q / WQ, h = t % H, d = t / H;
    const int dd = d - od, hh = h - oh, w0 = 4 * wq - ow;
    const int okr = (int)((unsigned)dd < (unsigned)D) & (int)((unsigned)hh < (unsigned)H);
    const int base = ((dd * H + hh) * W + w0) * 4;
    float v[4];
    if (ow == 0) {                               // wave-uniform branch: aligned row, one 16-byte load
      const float4 r = dca_bload4(dr, base, okr);
      v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = dca_bload1(dr, base + 4 * j, okr & (int)((unsigned)(w0 + j) < (unsigned)W));
    }
    *(float4*)(out + 4 * (long)q) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

int fill_args(C1Args& a, int N, int C, int D, int H, int W, const void* p0, const void* p1, const void* p2) {
  a.N = N; a.C = C; a.D = D; a.H = H; a.W = W;
  a.nTD = cdiv(D, TD); a.nTH = cdiv(H, TH); a.nTW = cdiv(W, TW);
  const long nt = (long)N * a.nTD * a.nTH * a.nTW;
  if (nt >= (1L << 31)) return 1;
  a.ntiles = (int)nt;
  a.vec = (W % 4 == 0) && ((((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) == 0);
  return 0;
}

// The launch of the two folded BatchNorm backward kernels.  Reduce: the chunking of bn_bwd_reduce_kernel (its partial count
// is the caller's, as for dca_bn_backward_pack), one workgroup per chunk and RCG channels.  Apply: persistent workgroups, 4 per
// CU (its 128 registers), each with at least two tiles where there are two.
struct C1BnGeom {
  DcaTileGrid t;
  int nchunk, nwg_apply;
  long chunk_len;
};
C1BnGeom c1_bn_geometry(int N, int D, int H, int W) {
  C1BnGeom g;
  g.t = dca_tile_grid<TD, TH, TW>(N, D, H, W);
  dca_internal_bn_chunking((long)D * H * W, BC, &g.nchunk, &g.chunk_len);
  const long cap = 4L * dca_num_cus(), half = g.t.tiles > 1 ? (g.t.tiles + 1) / 2 : 1;
  g.nwg_apply = (int)(half < cap ? half : cap);
  return g;
}
}  // namespace

extern "C" int dca_bn_backward_pack_c1_chunks(int N, int D, int H, int W) { return c1_bn_geometry(N, D, H, W).nchunk; }
extern "C" int dca_bn_backward_pack_c1_grid(int N, int D, int H, int W) { return c1_bn_geometry(N, D, H, W).nwg_apply; }

extern "C" int dca_bn_backward_pack_c1(const float* dlogit, const float* w_head, const float* y, const float* stats,
                                       double* part, float* dgb, void* dyp, int* dyexps, unsigned* gmax, const unsigned* ymax,
                                       int ymax_slots, int N, int C, int D, int H, int W, float slope, int training,
                                       hipStream_t stream) {
  DCA_REQUIRE(dlogit && w_head && y && stats && part && dgb && dyp && dyexps && gmax);
  DCA_REQUIRE(N > 0 && C == BC && D > 0 && H > 0 && W > 0 && W % 4 == 0);
  DCA_REQUIRE((long)C * D * H * W * 4 < 0x7ffffff0L);      // 32-bit byte offsets inside one sample
  DCA_REQUIRE(((((uintptr_t)dlogit) | ((uintptr_t)y) | ((uintptr_t)dyp)) & 15) == 0);
  DCA_REQUIRE(ymax == nullptr || (ymax_slots > 0 && ymax_slots <= DCA_AMAX_CSLOTS));
  const C1BnGeom g = c1_bn_geometry(N, D, H, W);
  DCA_REQUIRE(g.t.fits() && g.nchunk <= DCA_AMAX_CSLOTS);
  C1BnArgs a;
  a.dlogit = dlogit; a.y = y; a.stats = stats; a.dgb = dgb; a.dyexps = dyexps;
  a.part = part; a.gmax = gmax;
  a.N = N; a.D = D; a.H = H; a.W = W;
  a.nTD = g.t.nTD; a.nTH = g.t.nTH; a.nTW = g.t.nTW; a.ntiles = (int)g.t.tiles;
  a.slope = slope; a.training = training;
  hipLaunchKernelGGL(c1_bn_bwd_reduce_kernel, dim3(g.nchunk, BC / RCG), dim3(256), 0, stream, a, w_head, g.nchunk,
                     (int)g.chunk_len);
  const int rc = dca_internal_bn_bwd_finalize(part, g.nchunk, (double)N * (double)D * H * W, dgb, C, stats, training, gmax, ymax,
                                              ymax_slots, dyexps, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(c1_bn_bwd_apply_pack_kernel, dim3(g.nwg_apply), dim3(256), 0, stream, a, w_head, (char*)dyp);
  return dca_launch_status();
}

extern "C" int dca_conv3d_c1_bwd_data(const float* dy, const float* w, float* dx, int N, int C, int D, int H, int W,
                                      hipStream_t stream) {
  DCA_REQUIRE(dy && w && dx && N > 0 && C > 0 && C <= 256 && D > 0 && H > 0 && W > 0);
  C1Args a;
  a.x = nullptr; a.w = w; a.dy = dy; a.out = dx;
  DCA_REQUIRE(fill_args(a, N, C, D, H, W, dy, dx, nullptr) == 0);
  hipLaunchKernelGGL(c1_bwd_data_kernel, dim3(a.ntiles), dim3(256), (size_t)C * 36 * 4, stream, a);
  return dca_launch_status();
}

extern "C" int dca_conv3d_c1_gather(const float* T, float* y, int N, int D, int H, int W, hipStream_t stream) {
  DCA_REQUIRE(T && y && N > 0 && D > 0 && H > 0 && W > 0);
  DCA_REQUIRE(9L * D * H * W * 4 < 0x7ffffff0L && N <= 65535);  // 32-bit byte offsets inside one kd slab
  hipLaunchKernelGGL(c1_gather_kernel, dim3(cdiv((long)D * H * W, 1024), N), dim3(256), 0, stream, T, y, D, H, W);
  return dca_launch_status();
}

extern "C" int dca_conv3d_c1_expand(const float* dy, float* G, int N, int D, int H, int W, hipStream_t stream) {
  DCA_REQUIRE(dy && G && N > 0 && D > 0 && H > 0 && W > 0);
  DCA_REQUIRE((long)D * H * W * 4 < 0x7ffffff0L && N <= 65535);
  if (W % 4 == 0 && ((((uintptr_t)dy) | ((uintptr_t)G)) & 15) == 0) {
    hipLaunchKernelGGL(c1_expand4_kernel, dim3(cdiv((long)D * H * W / 4, 1024), 27, N), dim3(256), 0, stream, dy, G, D, H, W);
    return dca_launch_status();
  }
  hipLaunchKernelGGL(c1_expand_kernel, dim3(cdiv((long)D * H * W, 1024), 27, N), dim3(256), 0, stream, dy, G, D, H, W);
  return dca_launch_status();
}
