// Training inputs on the device (the reference's loaders after the decode, dataloader/datasets.py:221-254 SceneFlow and
// :270-317 KITTI): a uint8 pair and a raw disparity go in, the cropped, augmented, normalised fp32 batch slot, the
// ground-truth crop and its validity mask come out.
//   train_luma_sum     per image, the sum of PIL's convert("L") of the image after brightness and gamma (one byte table)
//   train_tables       sum -> contrast mean -> byte table U = contrast o gamma o brightness and float table T = norm o U
//   train_patch_colour per channel floor(mean) of the augmented right crop: the colour of the occlusion patch
//   train_crop_norm    the crop window through T into a planar fp32 batch slot, the patch rectangle filled with its colour
//   train_disp_crop    the crop window of the disparity (PFM row flip, KITTI 1/256, inf -> 0) and mask = 0 < gt < maxdisp
// Brightness, gamma and contrast are maps byte -> byte, so their composition is ONE 256-entry table per image; the only
// value that depends on the pixels is the contrast mean, and it comes from an exact integer sum.  Integer atomics only
// (order-free), no floating atomics: every result is bitwise reproducible.  Whatever one kernel derives from the data
// the next one reads from device memory: no host value is needed between the launches.
#include "dca_common.h"
#include "../../include/dca_hip.h"

#define TIO_THREADS 256
#define TIO_GROUP 48              // bytes per thread and step: 3 x 16-byte loads; 48 % 3 == 48 % 4 == 0
#define TIO_SUM_MAX_BLOCKS 48     // workgroups per image of the two summing kernels

// the operation order of train_tables is part of the contract (training.contrast_table restates it in numpy)
#pragma clang fp contract(off)

__device__ __forceinline__ unsigned long long tio_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// PIL's rgb2l (Convert.c): 19595 R + 38470 G + 7471 B + 0x8000 >> 16; at most 65536 * 255 + 32768 < 2^32
__device__ __forceinline__ unsigned tio_luma(unsigned r, unsigned g, unsigned b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

__device__ __forceinline__ unsigned tio_byte(const unsigned* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// ---- (a) luma sum -------------------------------------------------------------------------------------------------------
// grid (nblk, 2): image blockIdx.y.  Pixels [0, ngroups * 48 / C) are read as 16-byte words (the launcher passes
// ngroups = 0 for a base that is not 16-byte aligned), the rest one pixel at a time.  Per-thread totals are 64-bit: a
// 375 x 1242 all-255 image already sums to 1.2e8 and larger ones pass 2^32.
template <int C>
__global__ __launch_bounds__(TIO_THREADS) void train_luma_sum_kernel(const unsigned char* __restrict__ img0,
                                                                     const unsigned char* __restrict__ img1,
                                                                     const unsigned char* __restrict__ bg,
                                                                     unsigned long long* __restrict__ S, long npix,
                                                                     long ngroups0, long ngroups1) {
  __shared__ unsigned char tab[256];
  tab[threadIdx.x] = bg[blockIdx.y * 256 + threadIdx.x];          // TIO_THREADS == 256
  __syncthreads();
  const unsigned char* img = blockIdx.y ? img1 : img0;
  const long ngroups = blockIdx.y ? ngroups1 : ngroups0;
  constexpr int P = TIO_GROUP / C;                                // whole pixels per group
  const long gtid = (long)blockIdx.x * TIO_THREADS + threadIdx.x, gstride = (long)gridDim.x * TIO_THREADS;
  unsigned long long total = 0;
  for (long g = gtid; g < ngroups; g += gstride) {
    const uint4* p = (const uint4*)(img + g * TIO_GROUP);
    const uint4 a = p[0], b = p[1], c = p[2];
    const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    unsigned acc = 0;                                             // <= 16 * 255
#pragma unroll
    for (int q = 0; q < P; ++q)
      acc += tio_luma(tab[tio_byte(w, q * C)], tab[tio_byte(w, q * C + 1)], tab[tio_byte(w, q * C + 2)]);
    total += acc;
  }
  for (long q = ngroups * P + gtid; q < npix; q += gstride) {
    const unsigned char* s = img + q * C;
    total += tio_luma(tab[s[0]], tab[s[1]], tab[s[2]]);
  }
  total = tio_wave_sum(total);
  if ((threadIdx.x & 63) == 0 && total) atomicAdd(&S[blockIdx.y], total);
}
static_assert(TIO_THREADS == 256, "thread v stages entry v of the byte tables");

static inline unsigned tio_sum_blocks(long nbytes) {
  long nblk = (nbytes / TIO_GROUP + TIO_THREADS * 2 - 1) / (TIO_THREADS * 2);      // ~2 groups per thread
  return (unsigned)(nblk < 1 ? 1 : (nblk > TIO_SUM_MAX_BLOCKS ? TIO_SUM_MAX_BLOCKS : nblk));
}

extern "C" int dca_train_luma_sum(const unsigned char* left, const unsigned char* right, const unsigned char* bg,
                                  long long* S, int H, int W, int C, hipStream_t stream) {
  DCA_REQUIRE(left && right && bg && S && (C == 3 || C == 4) && H > 0 && W > 0);
  DCA_REQUIRE((long)H * W < (1L << 31));
  const long npix = (long)H * W, nbytes = npix * C;
  const long ng0 = ((uintptr_t)left & 15) ? 0 : nbytes / TIO_GROUP, ng1 = ((uintptr_t)right & 15) ? 0 : nbytes / TIO_GROUP;
  hipError_t rc = hipMemsetAsync(S, 0, 2 * sizeof(long long), stream);
  if (rc != hipSuccess) return (int)rc;
  const dim3 grid(tio_sum_blocks(nbytes), 2);
  if (C == 3)
    train_luma_sum_kernel<3><<<grid, TIO_THREADS, 0, stream>>>(left, right, bg, (unsigned long long*)S, npix, ng0, ng1);
  else
    train_luma_sum_kernel<4><<<grid, TIO_THREADS, 0, stream>>>(left, right, bg, (unsigned long long*)S, npix, ng0, ng1);
  return dca_launch_status();
}

// ---- (b) tables -----------------------------------------------------------------------------------------------------------
// PIL's ImagingBlend (Blend.c) of the constant image c and the value v: fp32, product then sum, no fma
__device__ __forceinline__ unsigned tio_blend(int c, int v, float f) {
  const float t = (float)c + f * (float)(v - c);
  if (f >= 0.f && f <= 1.f) return (unsigned)(int)t & 255u;      // t lies between c and v
  if (t <= 0.f) return 0u;
  if (t >= 255.f) return 255u;
  return (unsigned)(int)t;
}

// One workgroup; thread v writes entry v of the two byte tables and the six float tables.
__global__ __launch_bounds__(256) void train_tables_kernel(const long long* __restrict__ S, long n,
                                                           const unsigned char* __restrict__ bg, float f0, float f1,
                                                           const float* __restrict__ norm, unsigned char* __restrict__ U,
                                                           float* __restrict__ T) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // the sum another kernel's atomics left: a device-coherent vector load, not an s_load (dca_common.h)
    const long long Si = (long long)__hip_atomic_load((const unsigned long long*)&S[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int mean = (int)((double)Si / (double)n + 0.5);               // ImageEnhance.Contrast: int(ImageStat.mean + 0.5)
    mean = mean < 0 ? 0 : (mean > 255 ? 255 : mean);              // (a sum that fits n pixels never leaves the range)
    const unsigned u = tio_blend(mean, (int)bg[i * 256 + t], i ? f1 : f0);
    U[i * 256 + t] = (unsigned char)u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) T[(i * 3 + ch) * 256 + t] = norm[(i * 3 + ch) * 256 + u];
  }
}

extern "C" int dca_train_tables(const long long* S, long n_pixels, const unsigned char* bg, float f_left, float f_right,
                                const float* norm, unsigned char* U, float* T, hipStream_t stream) {
  DCA_REQUIRE(S && bg && norm && U && T && n_pixels > 0 && n_pixels < (1L << 31));
  DCA_REQUIRE(f_left - f_left == 0.f && f_right - f_right == 0.f);     // finite: inf * 0 in the blend would be NaN
  train_tables_kernel<<<1, 256, 0, stream>>>(S, n_pixels, bg, f_left, f_right, norm, U, T);
  return dca_launch_status();
}

// ---- (c) patch colour -------------------------------------------------------------------------------------------------------
// grid nblk: per-channel sums of U[1][byte] over the crop window of the right image (64-bit integer atomics into
// sums[3], zeroed by the launcher), then one small launch divides: floor(sum / (th tw)), what assigning numpy's mean to a
// uint8 array keeps.
__global__ __launch_bounds__(TIO_THREADS) void train_patch_sum_kernel(const unsigned char* __restrict__ right,
                                                                      const unsigned char* __restrict__ U,
                                                                      unsigned long long* __restrict__ sums, int W, int C,
                                                                      int y1, int x1, int th, int tw) {
  __shared__ unsigned char tab[256];
  tab[threadIdx.x] = U[256 + threadIdx.x];
  __syncthreads();
  const long n = (long)th * tw;
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (long i = (long)blockIdx.x * TIO_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * TIO_THREADS) {
    const int r = (int)(i / tw), c = (int)(i - (long)r * tw);
    const unsigned char* s = right + ((long)(y1 + r) * W + x1 + c) * C;
    const unsigned a = s[0], b = s[1], d = s[2];
    s0 += tab[a];
    s1 += tab[b];
    s2 += tab[d];
  }
  s0 = tio_wave_sum(s0);
  s1 = tio_wave_sum(s1);
  s2 = tio_wave_sum(s2);
  if ((threadIdx.x & 63) == 0) {
    if (s0) atomicAdd(&sums[0], s0);
    if (s1) atomicAdd(&sums[1], s1);
    if (s2) atomicAdd(&sums[2], s2);
  }
}

__global__ __launch_bounds__(64) void train_patch_final_kernel(const unsigned long long* __restrict__ sums,
                                                               unsigned char* __restrict__ colour, long n) {
  if (threadIdx.x < 3) colour[threadIdx.x] = (unsigned char)(sums[threadIdx.x] / (unsigned long long)n);
}

extern "C" int dca_train_patch_colour(const unsigned char* right, const unsigned char* U, long long* sums,
                                      unsigned char* colour, int H, int W, int C, int y1, int x1, int th, int tw,
                                      hipStream_t stream) {
  DCA_REQUIRE(right && U && sums && colour && (C == 3 || C == 4) && H > 0 && W > 0 && (long)H * W < (1L << 31));
  DCA_REQUIRE(y1 >= 0 && x1 >= 0 && th > 0 && tw > 0 && (long)y1 + th <= H && (long)x1 + tw <= W);
  hipError_t rc = hipMemsetAsync(sums, 0, 3 * sizeof(long long), stream);
  if (rc != hipSuccess) return (int)rc;
  const long n = (long)th * tw;
  train_patch_sum_kernel<<<tio_sum_blocks(n * 3), TIO_THREADS, 0, stream>>>(right, U, (unsigned long long*)sums, W, C, y1,
                                                                            x1, th, tw);
  train_patch_final_kernel<<<1, 64, 0, stream>>>((const unsigned long long*)sums, colour, n);
  return dca_launch_status();
}

// ---- (d) crop and normalise -----------------------------------------------------------------------------------------------
// grid (blocks over th * ceil(tw / V), 2): image blockIdx.y; a thread owns V consecutive columns of one crop row in all
// three planes.  Every cell of the grid lies inside the source window, so no load needs a guard or a redirect; the patch
// test comes after the loads and selects between the table entry and the patch value, so the 3 V byte loads are issued
// back to back.
template <int V>
__global__ __launch_bounds__(TIO_THREADS) void train_crop_norm_kernel(
    const unsigned char* __restrict__ img0, const unsigned char* __restrict__ img1, const float* __restrict__ T,
    const float* __restrict__ norm, const unsigned char* __restrict__ colour, float* __restrict__ out0,
    float* __restrict__ out1, int W, int C, int y1, int x1, int th, int tw, int py0, int px0, int ph, int pw) {
  __shared__ float tab[3 * 256];
  __shared__ float pv[3];
  for (int i = threadIdx.x; i < 3 * 256; i += TIO_THREADS) tab[i] = T[blockIdx.y * (3 * 256) + i];
  const bool patched = blockIdx.y == 1 && ph > 0 && pw > 0;      // the reference occludes the right image only
  if (threadIdx.x < 3) pv[threadIdx.x] = patched ? norm[(3 + threadIdx.x) * 256 + colour[threadIdx.x]] : 0.f;
  __syncthreads();
  const unsigned char* img = blockIdx.y ? img1 : img0;
  float* out = blockIdx.y ? out1 : out0;
  const int nxc = tw / V;                                         // V == 4 only when tw % 4 == 0
  const long cell = (long)blockIdx.x * TIO_THREADS + threadIdx.x;
  if (cell >= (long)th * nxc) return;
  const int y = (int)(cell / nxc), x0 = (int)(cell - (long)y * nxc) * V;
  const unsigned char* s = img + ((long)(y1 + y) * W + x1 + x0) * C;
  unsigned char px[V][3];
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[j][ch] = s[j * C + ch];
  const bool row_in = patched & (y >= py0) & (y < py0 + ph);
  float v[3][V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const bool in = row_in & (x0 + j >= px0) & (x0 + j < px0 + pw);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch][j] = in ? pv[ch] : tab[ch * 256 + px[j][ch]];
  }
  const long plane = (long)th * tw, o = (long)y * tw + x0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if (V == 4) {
      *(float4*)(out + ch * plane + o) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
    } else {
      out[ch * plane + o] = v[ch][0];
    }
  }
}

extern "C" int dca_train_crop_norm(const unsigned char* left, const unsigned char* right, const float* T, const float* norm,
                                   const unsigned char* colour, float* out_left, float* out_right, int H, int W, int C,
                                   int y1, int x1, int th, int tw, int py0, int px0, int ph, int pw, hipStream_t stream) {
  DCA_REQUIRE(left && right && T && out_left && out_right && (C == 3 || C == 4));
  DCA_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31) && th > 0 && tw > 0 && (long)th * tw < (1L << 31));
  DCA_REQUIRE(y1 >= 0 && x1 >= 0 && (long)y1 + th <= H && (long)x1 + tw <= W);
  DCA_REQUIRE(ph >= 0 && pw >= 0);
  if (ph > 0 && pw > 0) {
    DCA_REQUIRE(norm && colour && py0 >= 0 && px0 >= 0 && (long)py0 + ph <= th && (long)px0 + pw <= tw);
  }
  const bool vec = tw % 4 == 0 && (((uintptr_t)out_left | (uintptr_t)out_right) & 15) == 0;
  const long cells = (long)th * (vec ? tw / 4 : tw);
  const dim3 grid((unsigned)cdiv(cells, TIO_THREADS), 2);
  if (vec)
    train_crop_norm_kernel<4><<<grid, TIO_THREADS, 0, stream>>>(left, right, T, norm, colour, out_left, out_right, W, C, y1,
                                                                x1, th, tw, py0, px0, ph, pw);
  else
    train_crop_norm_kernel<1><<<grid, TIO_THREADS, 0, stream>>>(left, right, T, norm, colour, out_left, out_right, W, C, y1,
                                                                x1, th, tw, py0, px0, ph, pw);
  return dca_launch_status();
}

// ---- (e) disparity crop and mask --------------------------------------------------------------------------------------------
template <bool U16>
__global__ __launch_bounds__(TIO_THREADS) void train_disp_crop_kernel(const void* __restrict__ src, float* __restrict__ gt,
                                                                      unsigned char* __restrict__ mask, int H, int W, int y1,
                                                                      int x1, int th, int tw, int flip_rows, float scale,
                                                                      int inf_to_zero, float maxdisp) {
  const long n = (long)th * tw;
  for (long i = (long)blockIdx.x * TIO_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * TIO_THREADS) {
    const int r = (int)(i / tw), c = (int)(i - (long)r * tw);
    const int row = flip_rows ? H - 1 - (y1 + r) : y1 + r;        // a PFM payload is stored bottom-up
    const long idx = (long)row * W + x1 + c;
    float v;
    if (U16) {
      v = (float)((const unsigned short*)src)[idx] * scale;
    } else {
      v = ((const float*)src)[idx];
      if (scale != 1.f) v = v * scale;                            // scale 1: a bit copy, NaN payloads included
    }
    if (inf_to_zero && v == __builtin_inff()) v = 0.f;
    gt[i] = v;
    mask[i] = (v > 0.f && v < maxdisp) ? 1 : 0;                   // NaN: 0
  }
}

extern "C" int dca_train_disp_crop(const void* src, int src_u16, float* gt, unsigned char* mask, int H, int W, int y1,
                                   int x1, int th, int tw, int flip_rows, float scale, int inf_to_zero, float maxdisp,
                                   hipStream_t stream) {
  DCA_REQUIRE(src && gt && mask && H > 0 && W > 0 && (long)H * W < (1L << 31));
  DCA_REQUIRE(y1 >= 0 && x1 >= 0 && th > 0 && tw > 0 && (long)y1 + th <= H && (long)x1 + tw <= W);
  DCA_REQUIRE(((uintptr_t)src & (src_u16 ? 1 : 3)) == 0 && ((uintptr_t)gt & 3) == 0);
  const long n = (long)th * tw;
  long nblk = (n + TIO_THREADS - 1) / TIO_THREADS;
  nblk = nblk > 2048 ? 2048 : nblk;
  if (src_u16)
    train_disp_crop_kernel<true><<<(unsigned)nblk, TIO_THREADS, 0, stream>>>(src, gt, mask, H, W, y1, x1, th, tw, flip_rows,
                                                                             scale, inf_to_zero, maxdisp);
  else
    train_disp_crop_kernel<false><<<(unsigned)nblk, TIO_THREADS, 0, stream>>>(src, gt, mask, H, W, y1, x1, th, tw, flip_rows,
                                                                              scale, inf_to_zero, maxdisp);
  return dca_launch_status();
}
