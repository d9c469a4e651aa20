// Stereo visual odometry (nothing in the reference computes it): the motion of the left camera between
// two frames from the previous frame's disparity and the grey images of both, by inverse-compositional Gauss-Newton on a
// photometric error over a pyramid -- the definitions of include/dca_hip.h (dca_grey_pyramid, dca_disp_pyramid,
// dca_ego_motion) as they are written; the arithmetic is odometry_math.h's, shared with the host check.
//
// dca_ego_motion: one init launch, then per iteration
//  1. sums:  a persistent grid, at most one workgroup per CU, walks the source pixels of the level; 29 int64 sums per lane,
//            a cross-lane reduction, LDS across the waves, then ONE agent-scope relaxed INTEGER atomicAdd per (workgroup, sum).
//            Integer addition commutes: the same bits for every order.  No float atomic;
//  2. solve: one thread: the sums to fp64, LDL^T, the Cayley map, the composition, G of the next level and of level 0; it
//            clears the sums for the next iteration.
// Kernel boundaries are the only global synchronisation; what another kernel wrote (the record, G, the sums) is read with
// agent-scope loads.  Nothing is read back: the schedule is fixed, a failure is a flag in the record that
// makes every later launch return at once.
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "odometry_math.h"

#pragma clang fp contract(off)

namespace {

#define OD_THREADS 256
#define OD_WAVES (OD_THREADS / DCA_WAVE)
static_assert(OM_SUMS <= OD_THREADS && DCA_ODO_SUMS == OM_SUMS && DCA_ODO_REC_LEN >= 19, "the record and the sums of the header");

__device__ __forceinline__ double od_loadd(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ long long od_load64(const long long* p) {
  return (long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the pyramids: one thread per output pixel ---------------------------------------------------------------------------------
__global__ __launch_bounds__(OD_THREADS) void od_grey_kernel(const unsigned char* __restrict__ rgb, int C, long n,
                                                             unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * OD_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned char* p = rgb + i * C;
  out[i] = (unsigned char)(((int)p[0] + 2 * (int)p[1] + (int)p[2] + 2) >> 2);
}

__global__ __launch_bounds__(OD_THREADS) void od_grey_down_kernel(const unsigned char* __restrict__ src, int Ws, int Hd, int Wd,
                                                                  unsigned char* __restrict__ dst) {
  const long i = (long)blockIdx.x * OD_THREADS + threadIdx.x;
  if (i >= (long)Hd * Wd) return;
  const int r = (int)(i / Wd), c = (int)(i - (long)r * Wd);
  const unsigned char* p = src + (long)(2 * r) * Ws + 2 * c;        // 2 r + 1 < Hs and 2 c + 1 < Ws: Hd = Hs / 2, Wd = Ws / 2
  dst[i] = (unsigned char)(((int)p[0] + (int)p[1] + (int)p[Ws] + (int)p[Ws + 1] + 2) >> 2);
}

__global__ __launch_bounds__(OD_THREADS) void od_disp_copy_kernel(const float* __restrict__ src, long n, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * OD_THREADS + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(OD_THREADS) void od_disp_down_kernel(const float* __restrict__ src, int Ws, int Hd, int Wd,
                                                                  float min_disp, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * OD_THREADS + threadIdx.x;
  if (i >= (long)Hd * Wd) return;
  const int r = (int)(i / Wd), c = (int)(i - (long)r * Wd);
  const float* p = src + (long)(2 * r) * Ws + 2 * c;
  const float v[4] = {p[0], p[1], p[Ws], p[Ws + 1]};
  float m = 0.f;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool ok = fabsf(v[k]) < INFINITY && v[k] >= min_disp;
    m = ok && (!any || v[k] > m) ? v[k] : m;
    any = any || ok;
  }
  dst[i] = any ? m * 0.5f + 0.f : 0.f;                            // (+ 0: a -0.0, valid at min_disp = 0, leaves as +0.0)
}

// ---- the estimate ------------------------------------------------------------------------------------------------------------------
struct OdCam {
  double f, cx, cy;
};

struct OdInit {
  double t[12];                    // the host's start pose (metres); used without a device record
  OdCam first, zero;               // the cameras of the first (coarsest) level and of level 0
  double baseline;
  long out_words;                  // of sums_out
};

// one wave: thread 0 writes the record and both G, all threads clear the sums and sums_out
__global__ __launch_bounds__(DCA_WAVE) void od_init_kernel(OdInit a, const double* init_rec, double* rec, float* g, long long* sums,
                                                           long long* sums_out) {
  const int t = threadIdx.x;
  if (t < OM_SUMS) sums[t] = 0;
  if (sums_out)
    for (long i = t; i < a.out_words; i += DCA_WAVE) sums_out[i] = 0;
  if (t != 0) return;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tau[3] = {0.0, 0.0, 0.0};
  if (init_rec) {
    if (od_loadd(init_rec + 17) == 0.0) {                            // a failed estimate starts the next one from the identity
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = od_loadd(init_rec + 4 * i + j);
        tau[i] = od_loadd(init_rec + 12 + i);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R[3 * i + j] = a.t[4 * i + j];
      tau[i] = a.t[4 * i + 3] / a.baseline;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) rec[4 * i + j] = R[3 * i + j];
    rec[4 * i + 3] = tau[i] * a.baseline;
    rec[12 + i] = tau[i];
  }
#pragma unroll
  for (int i = 15; i < DCA_ODO_REC_LEN; ++i) rec[i] = 0.0;
  om_form_g(R, tau, a.zero.f, a.zero.cx, a.zero.cy, g);
  om_form_g(R, tau, a.first.f, a.first.cx, a.first.cy, g + 12);
}

__global__ __launch_bounds__(OD_THREADS) void od_sums_kernel(OmLevel L, const unsigned char* __restrict__ Ip,
                                                             const unsigned char* __restrict__ Ic, const float* __restrict__ D,
                                                             const double* rec, const float* g, long long* sums) {
  __shared__ long long part[OD_WAVES][OM_SUMS];
  if (od_loadd(rec + 17) != 0.0) return;                             // failed: the whole workgroup, the flag is one word
  const int t = threadIdx.x;
  float G[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) G[i] = dca_coherent_loadf(g + 12 + i);
  const int wi = L.W - 2;
  const long n = (L.H > 2 && wi > 0) ? (long)(L.H - 2) * wi : 0;
  long long S[OM_SUMS];
#pragma unroll
  for (int k = 0; k < OM_SUMS; ++k) S[k] = 0;
  for (long i = (long)blockIdx.x * OD_THREADS + t; i < n; i += (long)gridDim.x * OD_THREADS) {
    const int rr = (int)(i / wi), v = 1 + rr, u = 1 + (int)(i - (long)rr * wi);
    OmPixel p;
    if (om_pixel(L, G, Ip, Ic, D, u, v, &p)) om_accumulate(S, p);
  }
#pragma unroll
  for (int k = 0; k < OM_SUMS; ++k) {
#pragma unroll
    for (int o = DCA_WAVE / 2; o > 0; o >>= 1) S[k] += __shfl_xor(S[k], o, DCA_WAVE);
    if ((t & (DCA_WAVE - 1)) == 0) part[t / DCA_WAVE][k] = S[k];
  }
  __syncthreads();
  if (t < OM_SUMS) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < OD_WAVES; ++w) s += part[w][t];
    if (s != 0)
      __hip_atomic_fetch_add((unsigned long long*)(sums + t), (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct OdSolve {
  OdCam next, zero;                // the cameras of the next iteration's level and of level 0
  double baseline;
  int e[6];
  int min_pixels, slot;
};

__global__ __launch_bounds__(DCA_WAVE) void od_solve_kernel(OdSolve s, double* rec, float* g, long long* sums, long long* sums_out) {
  if (threadIdx.x != 0) return;
  if (od_loadd(rec + 17) != 0.0) return;
  long long S[OM_SUMS];
#pragma unroll
  for (int k = 0; k < OM_SUMS; ++k) {
    S[k] = od_load64(sums + k);
    sums[k] = 0;
    if (sums_out) sums_out[(long)s.slot * OM_SUMS + k] = S[k];
  }
  double R[9], tau[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = od_loadd(rec + 4 * i + j);
    tau[i] = od_loadd(rec + 12 + i);
  }
  rec[15] = (double)S[OM_N];
  rec[16] = om_residual(S);
  rec[18] = (double)(s.slot + 1);
  if (!om_update(S, s.e, s.min_pixels, R, tau)) {                     // the record keeps the last pose; G says "nothing"
    rec[17] = 1.0;
    const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int i = 0; i < 24; ++i) g[i] = nan;
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) rec[4 * i + j] = R[3 * i + j];
    rec[4 * i + 3] = tau[i] * s.baseline;
    rec[12 + i] = tau[i];
  }
  om_form_g(R, tau, s.zero.f, s.zero.cx, s.zero.cy, g);
  om_form_g(R, tau, s.next.f, s.next.cx, s.next.cy, g + 12);
}

// one thread: the world pose chained by the record's motion, and the frame's 35 doubles
__global__ __launch_bounds__(DCA_WAVE) void od_chain_kernel(const double* rec, double* world, double* out) {
  if (threadIdx.x != 0) return;
  double W[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double count = 0.0, residual = 0.0, status = 0.0;
  if (rec) {
#pragma unroll
    for (int i = 0; i < 12; ++i) W[i] = od_loadd(world + i);
    count = od_loadd(rec + 15), residual = od_loadd(rec + 16), status = od_loadd(rec + 17);
    if (status == 0.0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = od_loadd(rec + i);
      om_chain(W, T);
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) world[i] = W[i], out[i] = W[i], out[16 + i] = T[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) out[12 + i] = out[28 + i] = i == 3 ? 1.0 : 0.0;
  out[32] = count, out[33] = residual, out[34] = status;
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }
inline bool finite_d(double v) { return fabs(v) < (double)INFINITY; }
inline bool levels_ok(int H, int W, int levels) {
  return H > 0 && W > 0 && levels >= 1 && levels <= DCA_ODO_MAX_LEVELS && (H >> (levels - 1)) >= 1 && (W >> (levels - 1)) >= 1;
}
inline unsigned blocks_of(long n) { return (unsigned)((n + OD_THREADS - 1) / OD_THREADS); }

}  // namespace

extern "C" long dca_pyramid_len(int H, int W, int levels) {
  if (!levels_ok(H, W, levels) || (long)H * W >= (1L << 31)) return -1;
  long n = 0;
  for (int l = 0; l < levels; ++l) n += (long)(H >> l) * (W >> l);
  return n;
}

extern "C" int dca_grey_pyramid(const unsigned char* rgb, int H, int W, int C, int levels, unsigned char* out,
                                hipStream_t stream) {
  DCA_REQUIRE(rgb && out && (C == 3 || C == 4));
  DCA_REQUIRE(levels_ok(H, W, levels) && (long)H * W < (1L << 29));
  hipLaunchKernelGGL(od_grey_kernel, dim3(blocks_of((long)H * W)), dim3(OD_THREADS), 0, stream, rgb, C, (long)H * W, out);
  const unsigned char* src = out;
  for (int l = 1; l < levels; ++l) {
    const int Hs = H >> (l - 1), Ws = W >> (l - 1), Hd = H >> l, Wd = W >> l;
    unsigned char* dst = (unsigned char*)src + (long)Hs * Ws;
    hipLaunchKernelGGL(od_grey_down_kernel, dim3(blocks_of((long)Hd * Wd)), dim3(OD_THREADS), 0, stream, src, Ws, Hd, Wd, dst);
    src = dst;
  }
  return dca_launch_status();
}

extern "C" int dca_disp_pyramid(const float* disp, int H, int W, int levels, float min_disp, float* out, hipStream_t stream) {
  DCA_REQUIRE(disp && out && disp != out);
  DCA_REQUIRE(levels_ok(H, W, levels) && (long)H * W < (1L << 29));
  DCA_REQUIRE(min_disp >= 0.f && finite_f(min_disp));
  hipLaunchKernelGGL(od_disp_copy_kernel, dim3(blocks_of((long)H * W)), dim3(OD_THREADS), 0, stream, disp, (long)H * W, out);
  const float* src = out;
  for (int l = 1; l < levels; ++l) {
    const int Hs = H >> (l - 1), Ws = W >> (l - 1), Hd = H >> l, Wd = W >> l;
    float* dst = (float*)src + (long)Hs * Ws;
    hipLaunchKernelGGL(od_disp_down_kernel, dim3(blocks_of((long)Hd * Wd)), dim3(OD_THREADS), 0, stream, src, Ws, Hd, Wd, min_disp,
                       dst);
    src = dst;
  }
  return dca_launch_status();
}

extern "C" int dca_ego_motion(const unsigned char* prev, const unsigned char* cur, const float* disp, int H, int W, int levels,
                              int iters, double f, double baseline, double cx, double cy, double doffs, float min_disp,
                              float max_disp, float min_ratio, int grad_min, float huber, int min_pixels, const double* init_rec,
                              double t00, double t01, double t02, double t03, double t10, double t11, double t12, double t13,
                              double t20, double t21, double t22, double t23, double* rec, float* g, long long* sums,
                              long long* sums_out, hipStream_t stream) {
  DCA_REQUIRE(prev && cur && disp && rec && g && sums);
  DCA_REQUIRE(levels_ok(H, W, levels) && (long)H * W <= (1L << 20));               // the overflow budget of the int64 sums
  DCA_REQUIRE(iters >= 1 && iters <= DCA_ODO_MAX_ITERS);
  DCA_REQUIRE(finite_d(f) && f > 0.0 && finite_d(baseline) && baseline > 0.0 && finite_d(cx) && finite_d(cy) && finite_d(doffs) &&
              doffs >= 0.0);
  DCA_REQUIRE(min_disp >= 0.f && finite_f(min_disp) && finite_f(max_disp) && max_disp > min_disp && min_ratio > 0.f &&
              finite_f(min_ratio));
  DCA_REQUIRE(grad_min >= 0 && grad_min <= 510 && min_pixels >= 6);
  DCA_REQUIRE(finite_f(huber));
  const long huber_k = (long)rint((double)huber * 256.0);
  DCA_REQUIRE(huber_k >= 1 && huber_k <= 65280);
  DCA_REQUIRE(((uintptr_t)rec & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)sums_out & 7) == 0 && ((uintptr_t)g & 3) == 0);
  OdInit a = {{t00, t01, t02, t03, t10, t11, t12, t13, t20, t21, t22, t23}, {}, {}, baseline, (long)levels * iters * OM_SUMS};
  if (!init_rec)
    for (int i = 0; i < 12; ++i) DCA_REQUIRE(finite_d(a.t[i]));
  double dl;
  om_level_camera(f, cx, cy, doffs, levels - 1, &a.first.f, &a.first.cx, &a.first.cy, &dl);
  om_level_camera(f, cx, cy, doffs, 0, &a.zero.f, &a.zero.cx, &a.zero.cy, &dl);
  hipLaunchKernelGGL(od_init_kernel, dim3(1), dim3(DCA_WAVE), 0, stream, a, init_rec, rec, g, sums, sums_out);
  const int ncu = dca_num_cus();
  int slot = 0;
  for (int l = levels - 1; l >= 0; --l) {
    long off = 0;
    for (int k = 0; k < l; ++k) off += (long)(H >> k) * (W >> k);
    OdCam cam, next;
    double dn;
    om_level_camera(f, cx, cy, doffs, l > 0 ? l - 1 : 0, &next.f, &next.cx, &next.cy, &dn);
    om_level_camera(f, cx, cy, doffs, l, &cam.f, &cam.cx, &cam.cy, &dl);
    OmLevel L;
    L.f = (float)cam.f, L.cx = (float)cam.cx, L.cy = (float)cam.cy;
    L.doffs = (float)dl, L.min_disp = min_disp, L.max_disp = ldexpf(max_disp, -l), L.min_ratio = min_ratio;
    L.H = H >> l, L.W = W >> l, L.grad_min = grad_min, L.huber_k = (int)huber_k;
    OdSolve s = {cam, a.zero, baseline, {}, min_pixels, 0};
    om_exponents(cam.f, cam.cx, cam.cy, dl, (double)L.max_disp, L.H, L.W, s.e);
    for (int i = 0; i < 6; ++i) L.scale[i] = ldexpf(1.f, s.e[i]);
    const long n = (L.H > 2 && L.W > 2) ? (long)(L.H - 2) * (L.W - 2) : 0;
    long blocks = (n + OD_THREADS - 1) / OD_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > ncu ? ncu : blocks);
    for (int it = 0; it < iters; ++it, ++slot) {
      s.next = it + 1 < iters ? cam : next;
      s.slot = slot;
      hipLaunchKernelGGL(od_sums_kernel, dim3((unsigned)blocks), dim3(OD_THREADS), 0, stream, L, prev + off, cur + off, disp + off,
                         (const double*)rec, (const float*)g, sums);
      hipLaunchKernelGGL(od_solve_kernel, dim3(1), dim3(DCA_WAVE), 0, stream, s, rec, g, sums, sums_out);
    }
  }
  return dca_launch_status();
}

extern "C" int dca_pose_chain(const double* rec, double* world, double* out, hipStream_t stream) {
  DCA_REQUIRE(world && out && ((uintptr_t)rec & 7) == 0 && ((uintptr_t)world & 7) == 0 && ((uintptr_t)out & 7) == 0);
  hipLaunchKernelGGL(od_chain_kernel, dim3(1), dim3(DCA_WAVE), 0, stream, rec, world, out);
  return dca_launch_status();
}
