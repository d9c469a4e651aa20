// Stereo rectification of a raw camera pair on the device: ONE launch remaps both images through
// the fixed-point maps geometry.RectifyMaps built on the host from the calibration.
//   rectify_pair   per destination pixel a 4-tap bilinear gather with 5 fractional bits per axis, constant-zero border
// Integer arithmetic only, no atomics: the result is defined bit for bit (geometry.rectify_pair_host restates it in numpy).
#include "dca_common.h"
#include "../../include/dca_hip.h"

#define RECT_THREADS 256
#define RECT_V 4                  // destination pixels per thread: 16 bytes of X, 16 of Y, 12 (C = 3) or 16 (C = 4) of output

// Two horizontally adjacent source pixels, 2 C bytes from p, which need not be aligned: one dword and one short load for
// C = 3, two dwords for C = 4 (global loads take any address); the colour bytes of each pixel in the low 24 bits.
template <int C>
__device__ __forceinline__ void rect_load2(const unsigned char* __restrict__ p, unsigned& first, unsigned& second) {
  unsigned a;
  __builtin_memcpy(&a, p, 4);
  if (C == 4) {
    __builtin_memcpy(&second, p + 4, 4);
    first = a;
  } else {
    unsigned short b;
    __builtin_memcpy(&b, p + 4, 2);
    first = a & 0xFFFFFFu;
    second = (a >> 24) | ((unsigned)b << 8);
  }
}

// One source row's share of a destination pixel: taps (y, x0) and (y, x0 + 1) with the weights w0, w1, added into acc[3].
// The row is read as ONE pair of adjacent pixels q, q + 1 of the flat image, q clamped so that the pair lies inside it
// (n >= 2 pixels): a tap inside the source is pixel q or q + 1 (the clamp moves q only when the other tap is outside), a tap
// outside gets weight 0 whatever was loaded.  y and x0 are clamped before the product, so any int32 coordinate is safe.
template <int C>
__device__ __forceinline__ void rect_row(const unsigned char* __restrict__ img, const int y, const int x0, const int w0,
                                         const int w1, const int Hs, const int Ws, const int n, int (&acc)[3]) {
  const bool ry = (unsigned)y < (unsigned)Hs;
  const bool in0 = ry & ((unsigned)x0 < (unsigned)Ws), in1 = ry & ((unsigned)(x0 + 1) < (unsigned)Ws);
  const int f = min(max(y, 0), Hs - 1) * Ws + min(max(x0, -1), Ws - 1);      // in [-1, n - 1]
  const int q = min(max(f, 0), n - 2);
  unsigned first, second;
  rect_load2<C>(img + q * C, first, second);
  const unsigned t0 = f == q ? first : second, t1 = f + 1 == q ? first : second;
  const int u0 = in0 ? w0 : 0, u1 = in1 ? w1 : 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) acc[ch] += u0 * (int)((t0 >> (8 * ch)) & 255u) + u1 * (int)((t1 >> (8 * ch)) & 255u);
}

// the C bytes of the destination pixel with map entry (X, Y), packed into the low 8 C bits of the result
template <int C>
__device__ __forceinline__ unsigned rect_pixel(const unsigned char* __restrict__ img, const int X, const int Y, const int Hs,
                                               const int Ws, const int n) {
  const int x0 = X >> 5, a = X & 31, y0 = Y >> 5, b = Y & 31;      // arithmetic shift: floor for a negative coordinate
  int acc[3] = {512, 512, 512};
  if (n >= 2) {                                                    // uniform over the launch
    rect_row<C>(img, y0, x0, (32 - a) * (32 - b), a * (32 - b), Hs, Ws, n, acc);
    rect_row<C>(img, y0 + 1, x0, (32 - a) * b, a * b, Hs, Ws, n, acc);
  } else if ((x0 == -1 || x0 == 0) && (y0 == -1 || y0 == 0)) {      // a 1 x 1 source: the one tap that can be pixel (0, 0)
    const int w = (x0 ? a : 32 - a) * (y0 ? b : 32 - b);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += w * img[ch];
  }
  unsigned r = C == 4 ? 0xFF000000u : 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) r |= (unsigned)(acc[ch] >> 10) << (8 * ch);      // <= 255 each
  return r;
}

// grid (blocks over ceil(Hd Wd / RECT_V), 2): view blockIdx.y; a thread owns RECT_V consecutive destination pixels of the
// flat (row-major) index -- destination pixels do not depend on each other, so a group may run from the end of a row into
// the next and only the tail of the IMAGE is short.  maps: view-major planes X0, Y0, X1, Y1 of `plane` words each, `plane`
// a multiple of RECT_V, so a 16-byte aligned base makes every group's two loads aligned.  vec0 / vec1: the view's output
// base takes the group store (4-byte aligned for C = 3, 16-byte for C = 4) and the map base is 16-byte aligned.
template <int C>
__global__ __launch_bounds__(RECT_THREADS) void rectify_pair_kernel(
    const unsigned char* __restrict__ img0, const unsigned char* __restrict__ img1, const int* __restrict__ maps,
    unsigned char* __restrict__ out0, unsigned char* __restrict__ out1, int Hs, int Ws, int npix, int plane, int vec0,
    int vec1) {
  const unsigned char* img = blockIdx.y ? img1 : img0;
  unsigned char* out = blockIdx.y ? out1 : out0;
  const int* mx = maps + (long)blockIdx.y * 2 * plane;
  const int* my = mx + plane;
  const bool vec = blockIdx.y ? vec1 : vec0;
  const long g = (long)blockIdx.x * RECT_THREADS + threadIdx.x;
  const long i0 = g * RECT_V;
  const int n = Hs * Ws;
  if (i0 >= npix) return;
  if (vec && i0 + RECT_V <= npix) {
    const int4 X = *(const int4*)(mx + i0), Y = *(const int4*)(my + i0);
    const unsigned p0 = rect_pixel<C>(img, X.x, Y.x, Hs, Ws, n), p1 = rect_pixel<C>(img, X.y, Y.y, Hs, Ws, n);
    const unsigned p2 = rect_pixel<C>(img, X.z, Y.z, Hs, Ws, n), p3 = rect_pixel<C>(img, X.w, Y.w, Hs, Ws, n);
    if (C == 4) {
      *(uint4*)(out + i0 * 4) = make_uint4(p0, p1, p2, p3);
    } else {                                           // 4 x 3 bytes = three words
      unsigned* o = (unsigned*)(out + i0 * 3);
      o[0] = p0 | (p1 << 24);
      o[1] = (p1 >> 8) | (p2 << 16);
      o[2] = (p2 >> 16) | (p3 << 8);
    }
    return;
  }
  for (long i = i0; i < i0 + RECT_V && i < npix; ++i) {        // the image's tail, or a base the group store cannot take
    const unsigned p = rect_pixel<C>(img, mx[i], my[i], Hs, Ws, n);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[i * C + ch] = (unsigned char)(p >> (8 * ch));
  }
}

extern "C" int dca_rectify_pair(const unsigned char* left, const unsigned char* right, const int* maps, long map_plane,
                                unsigned char* out_left, unsigned char* out_right, int Hs, int Ws, int Hd, int Wd, int C,
                                hipStream_t stream) {
  DCA_REQUIRE(left && right && maps && out_left && out_right && (C == 3 || C == 4));
  DCA_REQUIRE(Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && Hs <= DCA_RECT_MAX_SRC && Ws <= DCA_RECT_MAX_SRC);
  DCA_REQUIRE((long)Hs * Ws * C < (1L << 31) && (long)Hd * Wd * C < (1L << 31));      // 32-bit offsets inside an image
  const long npix = (long)Hd * Wd;
  DCA_REQUIRE(map_plane >= npix && map_plane % RECT_V == 0 && map_plane < (1L << 31));
  const unsigned omask = C == 4 ? 15u : 3u;
  const bool mvec = ((uintptr_t)maps & 15) == 0;
  const int vec0 = mvec && ((uintptr_t)out_left & omask) == 0, vec1 = mvec && ((uintptr_t)out_right & omask) == 0;
  const dim3 grid((unsigned)cdiv(cdiv(npix, RECT_V), RECT_THREADS), 2);
  if (C == 3)
    rectify_pair_kernel<3><<<grid, RECT_THREADS, 0, stream>>>(left, right, maps, out_left, out_right, Hs, Ws, (int)npix,
                                                              (int)map_plane, vec0, vec1);
  else
    rectify_pair_kernel<4><<<grid, RECT_THREADS, 0, stream>>>(left, right, maps, out_left, out_right, Hs, Ws, (int)npix,
                                                              (int)map_plane, vec0, vec1);
  return dca_launch_status();
}
