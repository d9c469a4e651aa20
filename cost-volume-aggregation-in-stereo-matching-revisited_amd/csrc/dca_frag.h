// Matrix-core operand helpers shared by the convolution kernels: the 2-byte matrix types, the splits of an fp32 value into
// 2-byte terms (f16x2, bf16x3), the transposing LDS fragment read, and the weight layouts that the prep kernels write.
// One definition each: a packed operand or a weight image written by one kernel is read by others.
#pragma once
#include "dca_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef short s16x8 __attribute__((__vector_size__(8 * sizeof(short))));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ---- 2-byte matrix types MT = __bf16 / _Float16 -----------------------------------------------------------------------
// the 8-value MFMA operand and the 32x32x16 product
template <typename MT> struct Lp;
template <> struct Lp<__bf16> {
  typedef bf16x8 vec8;
  static __device__ __forceinline__ f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Lp<_Float16> {
  typedef f16x8 vec8;
  static __device__ __forceinline__ f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};
// conversion from fp32 (round to nearest even) to the raw 16-bit pattern, and back
template <typename MT> __device__ __forceinline__ unsigned short lp_bits(float v) {
  const MT m = (MT)v;
  return __builtin_bit_cast(unsigned short, m);
}
template <typename MT> __device__ __forceinline__ float lp_float(unsigned short b) {
  return (float)__builtin_bit_cast(MT, b);
}
// the low / high 2-byte value of a dword
template <typename MT> __device__ __forceinline__ float lp_lo(unsigned w) {
  return (float)__builtin_bit_cast(MT, (unsigned short)(w & 0xffffu));
}
template <typename MT> __device__ __forceinline__ float lp_hi(unsigned w) {
  return (float)__builtin_bit_cast(MT, (unsigned short)(w >> 16));
}
// two fp32 values -> one dword of two 2-byte values (lo = a, hi = b), round to nearest even (v_cvt_pk_*_f32)
template <typename MT> __device__ __forceinline__ unsigned lp_pack2(float a, float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef MT mtx2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, mtx2));
}

// ---- splits into 2-byte terms ------------------------------------------------------------------------------------------
// f16x2: v 2^e = h + l (+ <= 2^-22 relative); e from x2_scale_exp keeps the scaled maximum below 2^15.  The terms of the
// f16x2 kernels, and of the packed px2 operand format (dca_common.h) their producers write.
__device__ __forceinline__ void x2_split(float v, int e, _Float16& h, _Float16& l) {
  const float u = ldexpf(v, e);   // exact (v_ldexp_f32)
  h = (_Float16)u;
  l = (_Float16)(u - (float)h);   // the residual is exact in fp32
}

// The scales of an f16x2 weight image (x2_prep_weight_kernel, s2x2_prep_weight_kernel: workgroups of 512 threads, each
// packing 4 output channels of a block of CBLK): entry (o, k, tap) is stored as w 2^(f_o - xexps[k]), so these two rules are
// a contract with the forward kernels (ofo) and with the weight-gradient kernels that read xexps later.
// 1. xe[k] (LDS, k < A) = the operand's per-channel exponents: loaded from xexps when given, else derived from the
//    operand's per-channel maxima slots[k * DCA_AMAX_CSLOTS + s], s < nslots (16 threads per channel, 32 channels per round;
//    every workgroup derives its own copy) and written to xexps by workgroup 0.  The caller syncs before reading xe.
__device__ __forceinline__ void x2_prep_exps(int* xe, int A, const unsigned* __restrict__ slots, int nslots,
                                             int* __restrict__ xexps, int xexps_given) {
  const int tid = threadIdx.x;
  if (slots && !xexps_given) {
    for (int c0 = 0; c0 < A; c0 += 32) {
      const int c = c0 + (tid >> 4), l = tid & 15;
      unsigned v = 0;
      if (c < A)
        for (int i = l; i < nslots; i += 16) { const unsigned u = slots[(long)c * DCA_AMAX_CSLOTS + i]; v = v > u ? v : u; }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { const unsigned u = (unsigned)__shfl_xor((int)v, o, 64); v = v > u ? v : u; }
      if (c < A && l == 0) {
        const int e = x2_scale_exp(v);
        xe[c] = e;
        if (blockIdx.x == 0) xexps[c] = e;
      }
    }
  } else {
    for (int c = tid; c < A; c += 512) xe[c] = dca_coherent_loadi(xexps + c);
  }
}
// 2. f_o = 14 - max over (k, tap) of (exponent of w[o][k][tap]) - xe[k]: the row's largest scaled entry lands in
//    [2^14, 2^15); 0 for an all-zero row.  Row r = tid >> 7 (128 threads = 2 waves per output channel) is output channel
//    cblk * CBLK + r0 + r; f_o is left in rowmax[r][0] (LDS, synced) and written to ofo.
template <int CBLK>
__device__ __forceinline__ void x2_prep_row_scale(const float* __restrict__ src, int A, int Bn, int src_ab, const int* xe,
                                                  int (*rowmax)[2], int cblk, int r0, int* __restrict__ ofo) {
  const int tid = threadIdx.x;
  {
    const int r = tid >> 7, l = tid & 127, bi = cblk * CBLK + r0 + r;
    int m = -100000;
    if (bi < Bn) {
      for (int i = l; i < A * 27; i += 128) {
        const int ai = i / 27, tap = i - ai * 27;
        const float v = src_ab ? src[((long)ai * Bn + bi) * 27 + tap] : src[((long)bi * A + ai) * 27 + tap];
        const int be = (int)((__float_as_uint(v) >> 23) & 255);      // biased exponent; 0: zero / denormal -> ignored
        const int e = be == 0 ? -100000 : be - 127 - xe[ai];
        m = m > e ? m : e;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(m, o, 64); m = m > u ? m : u; }
    if ((l & 63) == 0) rowmax[r][l >> 6] = m;
  }
  __syncthreads();
  if (tid < 4) {
    const int m = rowmax[tid][0] > rowmax[tid][1] ? rowmax[tid][0] : rowmax[tid][1];
    const int fo = m <= -100000 ? 0 : 14 - m;
    rowmax[tid][0] = fo;
    ofo[cblk * CBLK + r0 + tid] = fo;
  }
  __syncthreads();
}

// bf16x3: v = h + m + l
__device__ __forceinline__ void x3_split(float v, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)v;
  const float r1 = v - (float)h;   // exact
  m = (__bf16)r1;
  const float r2 = r1 - (float)m;  // exact
  l = (__bf16)r2;
}
// term 0 / 1 / 2 = h / m / l of v, as its 16-bit pattern
__device__ __forceinline__ unsigned short x3_term_bits(float v, int term) {
  __bf16 h, m, l;
  x3_split(v, h, m, l);
  const __bf16 o = term == 0 ? h : (term == 1 ? m : l);
  return __builtin_bit_cast(unsigned short, o);
}

// 8 voxels x 1 channel f16 MFMA fragment from a [voxel][32 channels] LDS image: two transposing reads of 4 voxel rows each;
// the lane supplies the address of ITS row, `step` = bytes between the two blocks of four
__device__ __forceinline__ f16x8 tr_frag(const char* p, int step) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + step));
  const s16x8 c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(f16x8, c);
}

// ---- weight layouts: element idx of a prepared weight image, from a PyTorch weight --------------------------------------
// Written by the per-call prep kernels and by prep_many_kernel (one launch for a training step's whole set); a layout read
// by a kernel is the one defined here.  The source is src_ab ? src[a][b][K] : src[b][a][K] (a = contraction channel,
// b = output channel); flip reverses the tap order.  I is the index type of the caller's loop (int or long).

// fp32 image wt[tap][a < Apad][b < Bpad] of conv3d_mfma.hip, zero padded; b counts from b_off of Btotal source channels
template <typename I>
__device__ __forceinline__ float wt_f32_elem(const float* src, I idx, int A, int Bn, int Apad, int Bpad, int K, int src_ab,
                                             int flip, int Btotal, int b_off) {
  const int tap = (int)(idx / (Apad * Bpad)), ai = (int)((idx / Bpad) % Apad), bi = (int)(idx % Bpad);
  float v = 0.f;
  if (ai < A && bi < Bn) {
    const int st = flip ? K - 1 - tap : tap;
    v = src_ab ? src[((long)ai * Btotal + b_off + bi) * K + st] : src[((long)(b_off + bi) * A + ai) * K + st];
  }
  return v;
}

// bf16x3 fragments wx[cblk][chunk][tap][term][lane][j] of conv3d_bf16x3.hip (3x3x3, K = 27, NCH = ceil(A / 16)): lane
// (r = lane & 31, h = lane >> 5) holds A[row = output channel cblk*32 + r][k = input channel chunk*16 + 8h + j] of the tap,
// split into term 0/1/2 = h/m/l; zero padded
__device__ __forceinline__ unsigned short wx3_elem(const float* src, long idx, int A, int Bn, int NCH, int src_ab, int flip) {
  const int j = idx & 7, lane = (idx >> 3) & 63;
  long t = idx >> 9;
  const int term = t % 3; t /= 3;
  const int tap = t % 27; t /= 27;
  const int chunk = t % NCH;
  const int cblk = (int)(t / NCH);
  const int bi = cblk * 32 + (lane & 31), ai = chunk * 16 + 8 * (lane >> 5) + j;
  float v = 0.f;
  if (ai < A && bi < Bn) {
    const int st = flip ? 26 - tap : tap;
    v = src_ab ? src[((long)ai * Bn + bi) * 27 + st] : src[((long)bi * A + ai) * 27 + st];
  }
  return x3_term_bits(v, term);
}

// bf16x3 fragments wfrag[chunk][term][lane][j] of conv1_x3.hip (1x1x1, Bn <= 32): term of W[b = lane & 31][a = chunk*16 +
// 8*(lane >> 5) + j], W[b][a] = src_ab ? w[a*Btotal + b_off + b] : w[(b_off + b)*A + a]; zero for b >= Bn or a >= A
template <typename I>
__device__ __forceinline__ unsigned short w1x3_elem(const float* src, I idx, int A, int Bn, int src_ab, int Btotal, int b_off) {
  const int j = idx & 7, lane = (idx >> 3) & 63, term = (int)((idx >> 9) % 3), chunk = (int)((idx >> 9) / 3);
  const int bi = lane & 31, ai = chunk * 16 + 8 * (lane >> 5) + j;
  float v = 0.f;
  if (ai < A && bi < Bn) v = src_ab ? src[(long)ai * Btotal + b_off + bi] : src[(long)(b_off + bi) * A + ai];
  return x3_term_bits(v, term);
}
