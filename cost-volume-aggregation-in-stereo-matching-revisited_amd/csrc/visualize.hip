// Pictures of a disparity map on the device: the KITTI error map of a prediction against the ground
// truth (the reference's utils/visualization.py:11-55) and the colour-coded disparity map (the KITTI devkit's disp_to_color,
// or grey), as uint8 RGB next to the maps they are drawn from -- nothing returns to the host, nothing synchronises.
//   disp_error_image  one launch: crop by addressing, error, bin, colour, legend -> planar fp32 and / or interleaved uint8
//   disp_range        two launches: per-workgroup (min, max) of the valid pixels of a window, then one wave per image
//   disp_colorize     one launch: window of a map -> interleaved uint8, the range a host scalar or disp_range's pair
// Every thread owns four consecutive columns of one row: a 16-byte load per input where the row storage allows (width a
// multiple of 4, base 16-byte aligned), scalar loads otherwise and at the row's tail; the 12 bytes of four interleaved
// pixels leave as three dwords where they start on a dword, byte by byte otherwise.  No atomics: min and max do not depend
// on the order, every other result is per pixel, so everything is bitwise reproducible.
#include <math.h>

#include "dca_common.h"
#include "../../include/dca_hip.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define VIS_THREADS 256
#define VIS_RANGE_MAX_BLOCKS 128   // workgroups per image of dca_disp_range (= partial pairs per image)

__constant__ unsigned vis_err_rgb[DCA_ERRMAP_BINS] = {DCA_ERRMAP_RGB_0, DCA_ERRMAP_RGB_1, DCA_ERRMAP_RGB_2, DCA_ERRMAP_RGB_3,
                                                      DCA_ERRMAP_RGB_4, DCA_ERRMAP_RGB_5, DCA_ERRMAP_RGB_6, DCA_ERRMAP_RGB_7,
                                                      DCA_ERRMAP_RGB_8, DCA_ERRMAP_RGB_9};
static_assert(DCA_ERRMAP_BINS == 10, "ten rows in visualization.py:13-22");

// Four consecutive floats of a row from column x0 (a multiple of 4).  vec: the row starts on 16 bytes and its storage is a
// multiple of 4 wide, so x0 + 3 lies inside it -- one 16-byte load.  Otherwise the columns below `limit`, 0.0 elsewhere.
__device__ __forceinline__ void vis_load4(const float* __restrict__ row, int x0, int limit, bool vec, float v[4]) {
  if (vec) {
    const float4 q = *(const float4*)(row + x0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x0 + j < limit ? row[x0 + j] : 0.f;
  }
}

// The 0xRRGGBB words of pixels x0 .. x0 + 3 of a row of `w` pixels that starts at `dst`: three dwords when all four exist
// and the first byte lies on a dword, else the bytes of the pixels below w.
__device__ __forceinline__ void vis_put_rgb4(unsigned char* __restrict__ dst, int x0, int w, const unsigned rgb[4]) {
  unsigned char b[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    b[3 * j] = (unsigned char)(rgb[j] >> 16);
    b[3 * j + 1] = (unsigned char)(rgb[j] >> 8);
    b[3 * j + 2] = (unsigned char)rgb[j];
  }
  unsigned char* p = dst + 3L * x0;
  if (x0 + 3 < w && ((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      ((unsigned*)p)[k] = (unsigned)b[4 * k] | (unsigned)b[4 * k + 1] << 8 | (unsigned)b[4 * k + 2] << 16 | (unsigned)b[4 * k + 3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < w) {
        p[3 * j] = b[3 * j];
        p[3 * j + 1] = b[3 * j + 1];
        p[3 * j + 2] = b[3 * j + 2];
      }
  }
}

// ---- (a) error image -----------------------------------------------------------------------------------------------------------
// visualization.py:36-49 for one pixel: 0xRRGGBB of its bin, 0 outside the mask and for an error in no bin (NaN, +inf).
// np.minimum hands a NaN on, fminf would drop it.
__device__ __forceinline__ unsigned vis_err_colour(float g, float p, float abs_thres, float rel_thres) {
  if (!(g > 0.f)) return 0u;
  const float e = fabsf(g - p);
  const float a = e / abs_thres, r = (e / g) / rel_thres;
  const float err = (a != a || r != r) ? NAN : (a < r ? a : r);
  if (!(err >= 0.f && err < INFINITY)) return 0u;
  // edges 2^-4 .. 2^4: the bin is the number of edges at or below err
  const int bin = (err >= 0.0625f) + (err >= 0.125f) + (err >= 0.25f) + (err >= 0.5f) + (err >= 1.f) + (err >= 2.f) +
                  (err >= 4.f) + (err >= 8.f) + (err >= 16.f);
  return vis_err_rgb[bin];
}

// one thread per (image, row, four columns)
__global__ __launch_bounds__(VIS_THREADS) void disp_error_image_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, float* __restrict__ out_f32,
    unsigned char* __restrict__ out_u8, int B, int H, int W, int top_pad, int Wp, float abs_thres, float rel_thres,
    int legend, int vec_pred, int vec_gt, int vec_out) {
  const int nq = (W + 3) >> 2;
  const long cell = (long)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (cell >= (long)B * H * nq) return;
  const int q = (int)(cell % nq), r = (int)((cell / nq) % H), b = (int)(cell / ((long)nq * H));
  const int x0 = q * 4;
  float g[4], p[4];
  vis_load4(gt + ((long)b * H + r) * W, x0, W, vec_gt, g);
  vis_load4(pred + ((long)b * (H + top_pad) + top_pad + r) * Wp, x0, W, vec_pred, p);   // crop [:, top_pad:, :W] by addressing
  unsigned rgb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rgb[j] = vis_err_colour(g[j], p[j], abs_thres, rel_thres);
    const int x = x0 + j;
    if (legend && r < DCA_ERRMAP_LEGEND_ROWS && x < DCA_ERRMAP_LEGEND_STEP * DCA_ERRMAP_BINS)      // visualization.py:51-53
      rgb[j] = vis_err_rgb[x / DCA_ERRMAP_LEGEND_STEP];
  }
  if (out_u8) vis_put_rgb4(out_u8 + ((long)b * H + r) * W * 3, x0, W, rgb);
  if (out_f32) {
    const long plane = (long)H * W;
    float* o = out_f32 + (long)b * 3 * plane + (long)r * W + x0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)((rgb[j] >> (16 - 8 * ch)) & 255u) / 255.f;      // visualization.py:23
      if (vec_out) {
        *(float4*)(o + ch * plane) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) o[ch * plane + j] = v[j];
      }
    }
  }
}

// ---- (b) range -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vis_valid(float d, float m, bool has_mask, float mask_min) {
  return d > 0.f && d < INFINITY && (!has_mask || m >= mask_min);      // a NaN fails every comparison
}

// grid (nblk, B): every workgroup walks the four-column cells of one image's window and writes ONE (min, max) pair;
// (+inf, 0) when it saw no valid pixel
__global__ __launch_bounds__(VIS_THREADS) void disp_range_partial_kernel(const float* __restrict__ disp,
                                                                        const float* __restrict__ mask,
                                                                        float* __restrict__ part, int Hc, int Wc, int y0,
                                                                        int rows, int cols, float mask_min, int vec) {
  __shared__ float red[2][VIS_THREADS / 64];
  const int b = blockIdx.y, nq = (cols + 3) >> 2;
  const long frame = (long)b * Hc * Wc;
  float lo = INFINITY, hi = 0.f;
  for (int cell = blockIdx.x * VIS_THREADS + threadIdx.x; cell < rows * nq; cell += gridDim.x * VIS_THREADS) {   // rows nq < 2^31
    const int r = cell / nq, x0 = (cell - r * nq) * 4;
    const long row = frame + (long)(y0 + r) * Wc;
    float d[4], m[4] = {0.f, 0.f, 0.f, 0.f};
    vis_load4(disp + row, x0, cols, vec, d);
    if (mask) vis_load4(mask + row, x0, cols, vec, m);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < cols && vis_valid(d[j], m[j], mask != nullptr, mask_min)) {
        lo = fminf(lo, d[j]);
        hi = fmaxf(hi, d[j]);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lo;
    red[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < VIS_THREADS / 64; ++w) {
      lo = fminf(lo, red[0][w]);
      hi = fmaxf(hi, red[1][w]);
    }
    float* out = part + ((long)b * gridDim.x + blockIdx.x) * 2;
    out[0] = lo;
    out[1] = hi;
  }
}

// grid B, one wave: the partial pairs of image b -> range[b] = (lo, hi), (0, 0) without a valid pixel
__global__ __launch_bounds__(64) void disp_range_final_kernel(const float* __restrict__ part, float* __restrict__ range,
                                                              int nblk) {
  const int b = blockIdx.x;
  float lo = INFINITY, hi = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    lo = fminf(lo, part[((long)b * nblk + i) * 2]);
    hi = fmaxf(hi, part[((long)b * nblk + i) * 2 + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if (threadIdx.x == 0) {
    const bool any = hi > 0.f;          // a valid pixel is > 0
    range[2 * b] = any ? lo : 0.f;
    range[2 * b + 1] = any ? hi : 0.f;
  }
}

inline int vis_range_blocks(long cells) {
  const long n = (cells + (long)VIS_THREADS * 4 - 1) / ((long)VIS_THREADS * 4);
  return (int)(n < 1 ? 1 : (n > VIS_RANGE_MAX_BLOCKS ? VIS_RANGE_MAX_BLOCKS : n));
}

// ---- (c) colour-coded map ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned vis_byte(float v) { return (unsigned)rintf(v * 255.f); }      // v in [0, 1]

// the devkit's disp_to_color as include/dca_hip.h pins it in fp32; t in [0, 1]
__device__ __forceinline__ unsigned vis_kitti(float t) {
  constexpr float C[8] = {DCA_KITTI_EDGE_0, DCA_KITTI_EDGE_1, DCA_KITTI_EDGE_2, DCA_KITTI_EDGE_3,
                          DCA_KITTI_EDGE_4, DCA_KITTI_EDGE_5, DCA_KITTI_EDGE_6, DCA_KITTI_EDGE_7};
  const float s = t * 1000.f;
  int ind = 0;
  float c0 = C[0], wd = C[1] - C[0];
#pragma unroll
  for (int k = 1; k <= 6; ++k)
    if (s > C[k]) {
      ind = k;
      c0 = C[k];
      wd = C[k + 1] - C[k];      // the widths: integers, exact
    }
  const float w = (s - c0) / wd;
  const unsigned a = (DCA_KITTI_CORNERS >> (4 * ind)) & 7u, z = (DCA_KITTI_CORNERS >> (4 * ind + 4)) & 7u;   // bits r g b
  unsigned rgb = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned from = (a >> (2 - ch)) & 1u, to = (z >> (2 - ch)) & 1u;
    const float v = from == to ? (float)from : (to ? w : 1.f - w);
    rgb = rgb << 8 | vis_byte(v);
  }
  return rgb;
}

// one thread per (window row, four columns)
__global__ __launch_bounds__(VIS_THREADS) void disp_colorize_kernel(const float* __restrict__ disp,
                                                                   const float* __restrict__ mask,
                                                                   const float* __restrict__ range,
                                                                   unsigned char* __restrict__ out, int Wc, int y0, int rows,
                                                                   int cols, float max_disp, float mask_min, int cmap,
                                                                   int vec) {
  const int nq = (cols + 3) >> 2;
  const int cell = blockIdx.x * VIS_THREADS + threadIdx.x;
  if (cell >= rows * nq) return;
  const int r = cell / nq, x0 = (cell - r * nq) * 4;
  // the pair another launch wrote shortly before: a device-coherent vector load, not an s_load
  const float lo = range ? dca_coherent_loadf(range) : 0.f, hi = range ? dca_coherent_loadf(range + 1) : max_disp;
  const float span = fmaxf(hi - lo, 1e-5f);
  const long row = (long)(y0 + r) * Wc;
  float d[4], m[4] = {0.f, 0.f, 0.f, 0.f};
  vis_load4(disp + row, x0, cols, vec, d);
  if (mask) vis_load4(mask + row, x0, cols, vec, m);
  unsigned rgb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rgb[j] = 0u;
    if (vis_valid(d[j], m[j], mask != nullptr, mask_min)) {
      const float t = fminf(fmaxf((d[j] - lo) / span, 0.f), 1.f);
      rgb[j] = cmap == DCA_CMAP_KITTI ? vis_kitti(t) : vis_byte(t) * 0x010101u;
    }
  }
  vis_put_rgb4(out + (long)r * cols * 3, x0, cols, rgb);
}

inline bool vis_vec(const void* base, int width) { return width % 4 == 0 && ((uintptr_t)base & 15) == 0; }

}  // namespace

extern "C" int dca_disp_error_image(const float* pred, const float* gt, float* out_f32, unsigned char* out_u8, int B, int H,
                                    int W, int top_pad, int right_pad, float abs_thres, float rel_thres, int legend,
                                    hipStream_t stream) {
  DCA_REQUIRE(pred && gt && (out_f32 || out_u8));
  DCA_REQUIRE(B > 0 && H > 0 && W > 0 && top_pad >= 0 && right_pad >= 0 && (legend == 0 || legend == 1));
  DCA_REQUIRE((long)B * ((long)H + top_pad) * ((long)W + right_pad) < (1L << 31));
  DCA_REQUIRE(abs_thres > 0.f && abs_thres < INFINITY && rel_thres > 0.f && rel_thres < INFINITY);
  const int Wp = W + right_pad;
  const long cells = (long)B * H * ((W + 3) / 4);
  disp_error_image_kernel<<<(unsigned)cdiv(cells, VIS_THREADS), VIS_THREADS, 0, stream>>>(
      pred, gt, out_f32, out_u8, B, H, W, top_pad, Wp, abs_thres, rel_thres, legend, vis_vec(pred, Wp), vis_vec(gt, W),
      vis_vec(out_f32, W));
  return dca_launch_status();
}

extern "C" long dca_disp_range_workspace(int B, int rows, int cols) {
  if (B <= 0 || rows <= 0 || cols <= 0 || (long)rows * cols >= (1L << 31)) return 0;
  return (long)B * vis_range_blocks((long)rows * ((cols + 3) / 4)) * 2 * (long)sizeof(float);
}

extern "C" int dca_disp_range(const float* disp, const float* mask, float* range, void* workspace, int B, int Hc, int Wc,
                              int y0, int rows, int cols, float mask_min, hipStream_t stream) {
  DCA_REQUIRE(disp && range && workspace && B > 0 && B <= 65535);
  DCA_REQUIRE(dca_window_ok(Hc, Wc, y0, rows, cols) && (long)B * Hc * Wc < (1L << 31) && (!mask || mask_min == mask_min));
  const int nblk = vis_range_blocks((long)rows * ((cols + 3) / 4));
  const int vec = vis_vec(disp, Wc) && (!mask || vis_vec(mask, Wc));
  disp_range_partial_kernel<<<dim3(nblk, B), VIS_THREADS, 0, stream>>>(disp, mask, (float*)workspace, Hc, Wc, y0, rows, cols,
                                                                       mask_min, vec);
  disp_range_final_kernel<<<B, 64, 0, stream>>>((const float*)workspace, range, nblk);
  return dca_launch_status();
}

extern "C" int dca_disp_colorize(const float* disp, const float* mask, const float* range, unsigned char* out_u8, int Hc,
                                 int Wc, int y0, int rows, int cols, float max_disp, float mask_min, int cmap,
                                 hipStream_t stream) {
  DCA_REQUIRE(disp && out_u8 && (cmap == DCA_CMAP_GRAY || cmap == DCA_CMAP_KITTI));
  DCA_REQUIRE(dca_window_ok(Hc, Wc, y0, rows, cols) && (!mask || mask_min == mask_min));
  DCA_REQUIRE(range || (max_disp > 0.f && max_disp < INFINITY));
  const int vec = vis_vec(disp, Wc) && (!mask || vis_vec(mask, Wc));
  const long cells = (long)rows * ((cols + 3) / 4);
  disp_colorize_kernel<<<(unsigned)cdiv(cells, VIS_THREADS), VIS_THREADS, 0, stream>>>(disp, mask, range, out_u8, Wc, y0, rows,
                                                                                       cols, max_disp, mask_min, cmap, vec);
  return dca_launch_status();
}
