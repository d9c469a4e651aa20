// Frame I/O of the inference step (my_img.py:47-110) on the device: a uint8 camera pair goes in, the normalised, padded
// fp32 frames the network reads come out, and the network's disparity leaves as the cropped fp32 / KITTI uint16 image.
//   frame_hist   per image and colour plane, the histogram of the 256 byte values      (integer atomics: order-free)
//   frame_lut    histogram -> mean, population std (fp64, fixed operation order) -> 256-entry table (v - mean) / std
//   frame_apply  table look-up + placement in the zero-padded frame; writes EVERY frame element
//   disp_export  window of the prediction as fp32 (bit copy) and / or uint16(pred * scale)
// A uint8 plane has 256 distinct values, so the table holds every value the host normalisation can produce; the
// statistics come from exact integer counts.  No floating atomics anywhere: every result is bitwise reproducible.
#include "dca_common.h"
#include "../../include/dca_hip.h"

#define FIO_THREADS 256
#define FIO_WAVES (FIO_THREADS / 64)
#define FIO_REP 4                 // sub-histograms per wave: lane l counts in copy l % FIO_REP
#define FIO_GROUP 48              // bytes per thread and step: 3 x 16-byte loads; 48 % 3 == 48 % 4 == 0
#define FIO_HIST_MAX_BLOCKS 48    // workgroups per image
#define FIO_BINS (3 * 256)

// ---- (a) histogram ---------------------------------------------------------------------------------------------------
// Every wave owns FIO_REP copies of the 3 x 256 counters, interleaved so that copy r of bin b is word b * FIO_REP + r:
// natural images pile neighbouring lanes onto the same few bins, and with the copies side by side those lanes hit
// FIO_REP different words on FIO_REP different banks instead of serialising on one.
template <int C>
__device__ __forceinline__ void fio_count16(unsigned* __restrict__ h, const uint4 q, const int k0) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int ch = (k0 + k) % C;                 // compile-time after unrolling: the group starts at a multiple of C
    if (ch < 3) atomicAdd(&h[(ch * 256 + ((w[k >> 2] >> (8 * (k & 3))) & 255u)) * FIO_REP], 1u);
  }
}

// grid (nblk, 2): image blockIdx.y.  Bytes [0, ngroups * 48) are read as 16-byte words (the launcher passes ngroups = 0
// for a base that is not 16-byte aligned), the rest one byte at a time.
template <int C>
__global__ __launch_bounds__(FIO_THREADS) void frame_hist_kernel(const unsigned char* __restrict__ img0,
                                                                 const unsigned char* __restrict__ img1,
                                                                 unsigned* __restrict__ hist, long nbytes, long ngroups0,
                                                                 long ngroups1) {
  __shared__ unsigned lh[FIO_WAVES * FIO_BINS * FIO_REP];
  for (int i = threadIdx.x; i < FIO_WAVES * FIO_BINS * FIO_REP; i += FIO_THREADS) lh[i] = 0;
  __syncthreads();
  const unsigned char* img = blockIdx.y ? img1 : img0;
  const long ngroups = blockIdx.y ? ngroups1 : ngroups0;
  unsigned* h = lh + (threadIdx.x >> 6) * (FIO_BINS * FIO_REP) + (threadIdx.x & (FIO_REP - 1));
  const long gtid = (long)blockIdx.x * FIO_THREADS + threadIdx.x, gstride = (long)gridDim.x * FIO_THREADS;
  for (long g = gtid; g < ngroups; g += gstride) {
    const uint4* p = (const uint4*)(img + g * FIO_GROUP);
    const uint4 a = p[0], b = p[1], c = p[2];
    fio_count16<C>(h, a, 0);
    fio_count16<C>(h, b, 16);
    fio_count16<C>(h, c, 32);
  }
  for (long i = ngroups * FIO_GROUP + gtid; i < nbytes; i += gstride) {
    const int ch = (int)(i % C);
    if (ch < 3) atomicAdd(&h[(ch * 256 + img[i]) * FIO_REP], 1u);
  }
  __syncthreads();
  unsigned* out = hist + blockIdx.y * FIO_BINS;
  for (int b = threadIdx.x; b < FIO_BINS; b += FIO_THREADS) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < FIO_WAVES; ++w) {
      const uint4 v = *(const uint4*)&lh[w * (FIO_BINS * FIO_REP) + b * FIO_REP];   // FIO_REP == 4 copies, one 16-byte read
      n += v.x + v.y + v.z + v.w;
    }
    if (n) atomicAdd(&out[b], n);
  }
}
static_assert(FIO_REP == 4, "the merge reads the copies of a bin as one uint4");

extern "C" int dca_frame_hist(const unsigned char* left, const unsigned char* right, unsigned* hist, int H, int W, int C,
                              hipStream_t stream) {
  DCA_REQUIRE(left && right && hist && (C == 3 || C == 4) && H > 0 && W > 0);
  DCA_REQUIRE((long)H * W < (1L << 31));
  const long nbytes = (long)H * W * C;
  const long ng0 = ((uintptr_t)left & 15) ? 0 : nbytes / FIO_GROUP, ng1 = ((uintptr_t)right & 15) ? 0 : nbytes / FIO_GROUP;
  hipError_t rc = hipMemsetAsync(hist, 0, 2 * FIO_BINS * sizeof(unsigned), stream);
  if (rc != hipSuccess) return (int)rc;
  long nblk = (nbytes / FIO_GROUP + FIO_THREADS * 2 - 1) / (FIO_THREADS * 2);      // ~2 groups per thread
  nblk = nblk < 1 ? 1 : (nblk > FIO_HIST_MAX_BLOCKS ? FIO_HIST_MAX_BLOCKS : nblk);
  if (C == 3)
    frame_hist_kernel<3><<<dim3((unsigned)nblk, 2), FIO_THREADS, 0, stream>>>(left, right, hist, nbytes, ng0, ng1);
  else
    frame_hist_kernel<4><<<dim3((unsigned)nblk, 2), FIO_THREADS, 0, stream>>>(left, right, hist, nbytes, ng0, ng1);
  return dca_launch_status();
}

// ---- (b) histogram -> table ---------------------------------------------------------------------------------------------
// One workgroup.  Thread p < 6 walks the 256 bins of plane p in order (the operation order is part of the contract:
// inference.lut_from_histogram restates it in numpy and must match bit for bit, hence no contraction into fma);
// then thread v writes entry v of the six tables.
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void frame_lut_kernel(const unsigned* __restrict__ hist, float* __restrict__ lut,
                                                        double* __restrict__ stats, long n) {
  __shared__ double ms[6][2];
  const int t = threadIdx.x;
  if (t < 6) {
    const unsigned* h = hist + t * 256;
    unsigned long long S = 0;
    for (int v = 0; v < 256; ++v) S += (unsigned long long)h[v] * (unsigned)v;
    const double mean = (double)S / (double)n;
    double acc = 0.0;
    for (int v = 0; v < 256; ++v) {
      const double d = (double)v - mean;
      acc = acc + (double)h[v] * (d * d);
    }
    const double sd = __dsqrt_rn(acc / (double)n);
    ms[t][0] = mean;
    ms[t][1] = sd;
    stats[t * 2] = mean;
    stats[t * 2 + 1] = sd;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 6; ++p) lut[p * 256 + t] = (float)(((double)t - ms[p][0]) / ms[p][1]);   // std = 0: 0/0 = NaN, x/0 = inf, as numpy
}

extern "C" int dca_frame_lut(const unsigned* hist, long n_pixels, float* lut, double* stats, hipStream_t stream) {
  DCA_REQUIRE(hist && lut && stats && n_pixels > 0 && n_pixels < (1L << 31));
  frame_lut_kernel<<<1, 256, 0, stream>>>(hist, lut, stats, n_pixels);
  return dca_launch_status();
}

// ---- (c) table look-up + placement ----------------------------------------------------------------------------------------
// grid (blocks over Hc * ceil(Wc / V), 2): image blockIdx.y; a thread owns V consecutive frame columns of one row in all
// three planes.  Inside the window the value is the table entry of the source byte, everywhere else +0.0.
template <int V>
__global__ __launch_bounds__(FIO_THREADS) void frame_apply_kernel(
    const unsigned char* __restrict__ img0, const unsigned char* __restrict__ img1, const float* __restrict__ lut,
    float* __restrict__ out0, float* __restrict__ out1, int W, int C, int Hc, int Wc, int src_y0, int dst_y0, int rows,
    int cols) {
  __shared__ float tab[FIO_BINS];
  for (int i = threadIdx.x; i < FIO_BINS; i += FIO_THREADS) tab[i] = lut[blockIdx.y * FIO_BINS + i];
  __syncthreads();
  const unsigned char* img = blockIdx.y ? img1 : img0;
  float* out = blockIdx.y ? out1 : out0;
  const int nxc = (Wc + V - 1) / V;
  const long cell = (long)blockIdx.x * FIO_THREADS + threadIdx.x;
  if (cell >= (long)Hc * nxc) return;
  const int y = (int)(cell / nxc), x0 = (int)(cell - (long)y * nxc) * V;
  const int sy = y - dst_y0 + src_y0;
  const bool row_in = y >= dst_y0 && y < dst_y0 + rows;
  // outside the window the loads go to pixel 0 of the image and their result is dropped: no branch around a load, so
  // the 3 V byte loads are issued back to back
  unsigned char px[V][3];
  bool in[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    in[j] = row_in & (x0 + j < cols);
    const unsigned char* s = img + (in[j] ? ((long)sy * W + x0 + j) * C : 0L);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[j][ch] = s[ch];
  }
  float v[3][V];
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch][j] = in[j] ? tab[ch * 256 + px[j][ch]] : 0.f;
  const long plane = (long)Hc * Wc, o = (long)y * Wc + x0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if (V == 4) {
      *(float4*)(out + ch * plane + o) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
    } else {
      out[ch * plane + o] = v[ch][0];
    }
  }
}

extern "C" int dca_frame_apply(const unsigned char* left, const unsigned char* right, const float* lut, float* out_left,
                               float* out_right, int H, int W, int C, int Hc, int Wc, int src_y0, int dst_y0, int rows,
                               int cols, hipStream_t stream) {
  DCA_REQUIRE(left && right && lut && out_left && out_right && (C == 3 || C == 4));
  DCA_REQUIRE(H > 0 && W > 0 && Hc > 0 && Wc > 0 && (long)H * W < (1L << 31) && (long)Hc * Wc < (1L << 31));
  DCA_REQUIRE(src_y0 >= 0 && dst_y0 >= 0 && rows >= 0 && cols >= 0);
  DCA_REQUIRE((long)src_y0 + rows <= H && cols <= W && (long)dst_y0 + rows <= Hc && cols <= Wc);
  const bool vec = Wc % 4 == 0 && (((uintptr_t)out_left | (uintptr_t)out_right) & 15) == 0;
  const long cells = (long)Hc * (vec ? Wc / 4 : Wc);
  const dim3 grid((unsigned)cdiv(cells, FIO_THREADS), 2);
  if (vec)
    frame_apply_kernel<4><<<grid, FIO_THREADS, 0, stream>>>(left, right, lut, out_left, out_right, W, C, Hc, Wc, src_y0,
                                                            dst_y0, rows, cols);
  else
    frame_apply_kernel<1><<<grid, FIO_THREADS, 0, stream>>>(left, right, lut, out_left, out_right, W, C, Hc, Wc, src_y0,
                                                            dst_y0, rows, cols);
  return dca_launch_status();
}

// ---- (d) disparity export -------------------------------------------------------------------------------------------------
// uint16(pred * scale): dca_sat_u16 (dca_common.h)
__global__ __launch_bounds__(FIO_THREADS) void disp_export_kernel(const unsigned* __restrict__ pred,
                                                                  unsigned* __restrict__ out_f32,
                                                                  unsigned short* __restrict__ out_u16, int Wc, int y0,
                                                                  int h, int w, float scale) {
  const long n = (long)h * w;
  for (long i = (long)blockIdx.x * FIO_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * FIO_THREADS) {
    const int r = (int)(i / w), c = (int)(i - (long)r * w);
    const unsigned bits = pred[(long)(y0 + r) * Wc + c];
    if (out_f32) out_f32[i] = bits;
    if (out_u16) out_u16[i] = dca_sat_u16(__uint_as_float(bits) * scale);
  }
}

extern "C" int dca_disp_export(const float* pred, float* out_f32, unsigned short* out_u16, int Hc, int Wc, int y0, int h,
                               int w, float scale, hipStream_t stream) {
  DCA_REQUIRE(pred && (out_f32 || out_u16));
  DCA_REQUIRE(dca_window_ok(Hc, Wc, y0, h, w));
  const long n = (long)h * w;
  long nblk = (n + FIO_THREADS - 1) / FIO_THREADS;
  nblk = nblk > 2048 ? 2048 : nblk;
  disp_export_kernel<<<(unsigned)nblk, FIO_THREADS, 0, stream>>>((const unsigned*)pred, (unsigned*)out_f32, out_u16, Wc, y0,
                                                                  h, w, scale);
  return dca_launch_status();
}
