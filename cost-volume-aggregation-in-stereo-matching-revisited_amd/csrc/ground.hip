// Ground plane, obstacles and free space from disparity (nothing in the reference computes it): the
// definitions of include/dca_hip.h (dca_ground_plane, dca_ground_segment) as they are written, the arithmetic itself in
// ground_math.h, which the host check tools/ground_math_check.cpp compiles too.
//
// dca_ground_plane, 2 + 2 refine launches (3 for refine = 0), the kernel boundaries being the only global synchronisation:
//  1. vdisp:  one wave per window row, the row's NB bins in LDS (integer adds), then every bin stored once: vdisp needs no
//             clearing and sees no global atomic.  Workgroup 0 of every image clears the image's workspace words.
//  2. vote:   one thread per candidate (d_top, d_bot), consecutive lanes consecutive d_top, so the lanes of a wave read
//             neighbouring bins of one row of vdisp (L2-resident: NB words per fit row).  The key's maximum over the
//             workgroup, then ONE agent-scope 64-bit integer atomicMax per workgroup.
//  3. sums:   the inliers of the round, ten int64 sums per thread, per wave (shuffles), per workgroup (LDS), then ten
//             agent-scope integer adds per workgroup.  Integer addition is associative: the sums are exact, any order.
//  4. solve:  one thread per image: key -> Hough line (round 0), sums -> gm_solve -> the record.
// dca_ground_segment, two launches:
//  1. column: one lane per column walks it from the bottom row up (coalesced across the lanes) for the obstacle's base; the
//             launch also clears bev, which only the next launch adds to.
//  2. pixel:  one thread per pixel: label, height, and the cell of bev.  A run of consecutive lanes that hit the same cell
//             (neighbouring road pixels do) sends ONE integer atomic with the run's length.
// Scalars another kernel wrote (the key, the sums, the record) are read with device-coherent vector loads.
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "ground_math.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define GR_THREADS 256
#define GR_WAVES (GR_THREADS / DCA_WAVE)
#define GR_MAX_BLOCKS 1024
static_assert(DCA_GROUND_WS_LEN <= GR_THREADS && DCA_GROUND_WS_LEN >= 8 + GM_SUMS * DCA_GROUND_MAX_REFINE, "workspace layout");
static_assert(DCA_GROUND_PLANE_LEN == 16, "record layout");

// B maps (B,Hc,Wc) with the window rows x cols at frame row y0, column 0 of every image
struct GrFrame {
  const float* d;
  const float* mask;                                         // indexed like d, or NULL
  int Hc, Wc, y0, rows, cols, NB;
  float min_disp, mask_min;
  __device__ __forceinline__ long at(int b, int r, int c) const { return ((long)b * Hc + (y0 + r)) * (long)Wc + c; }
  __device__ __forceinline__ bool valid(long i, float& v, int& q) const {
    v = d[i];
    return gm_valid(v, min_disp, NB, &q) && (!mask || mask[i] >= mask_min);
  }
};

__device__ __forceinline__ unsigned long long coherent_load64(const void* p) {
  return __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double coherent_loadd(const double* p) { return __longlong_as_double((long long)coherent_load64(p)); }

// ---- 1. v-disparity: grid (ceil(rows / GR_WAVES), B) ----------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void gp_vdisp_kernel(GrFrame f, int* __restrict__ vdisp, long long* __restrict__ ws) {
  __shared__ int hist[GR_WAVES * DCA_GROUND_MAX_DISP];
  const int t = threadIdx.x, lane = t & (DCA_WAVE - 1), w = t / DCA_WAVE, b = blockIdx.y;
  const int r = blockIdx.x * GR_WAVES + w;
  int* h = hist + w * f.NB;
  for (int k = lane; k < f.NB; k += DCA_WAVE) h[k] = 0;
  __syncthreads();
  if (r < f.rows) {
    for (int c = lane; c < f.cols; c += DCA_WAVE) {
      float v;
      int q;
      if (f.valid(f.at(b, r, c), v, q)) atomicAdd(&h[q >> 4], 1);
    }
  }
  __syncthreads();
  if (r < f.rows) {
    int* out = vdisp + ((long)b * f.rows + r) * f.NB;
    for (int k = lane; k < f.NB; k += DCA_WAVE) out[k] = h[k];
  }
  if (blockIdx.x == 0 && t < DCA_GROUND_WS_LEN) ws[(long)b * DCA_GROUND_WS_LEN + t] = 0;
}

// ---- 2. Hough vote: grid (ceil(ncand / GR_THREADS), B), ncand = (NB - 1) 2 NB ------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void gp_vote_kernel(const int* __restrict__ vdisp, long long* ws, int rows, int NB,
                                                             int r_lo, int r_hi, int min_rise, int ncand) {
  __shared__ unsigned long long best[GR_WAVES];
  const int t = threadIdx.x, j = blockIdx.x * GR_THREADS + t, b = blockIdx.y;
  unsigned long long key = 0;                                // below every candidate's key (~index is never 0 in 32 bits)
  if (j < ncand) {
    const int d_bot = 1 + j / (2 * NB), d_top = j % (2 * NB) - NB;
    if (d_bot - d_top >= min_rise) {
      const int* v = vdisp + (long)b * rows * NB;
      int vote = 0;
      for (int r = r_lo; r < r_hi; ++r) {
        const int bin = gm_line_bin(d_top, d_bot, r, rows);
        if (bin >= 0 && bin < NB) vote += v[(long)r * NB + bin];
      }
      key = gm_hough_key(vote, d_top, d_bot, NB);
    }
  }
#pragma unroll
  for (int o = DCA_WAVE / 2; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, DCA_WAVE);
    key = other > key ? other : key;
  }
  if ((t & (DCA_WAVE - 1)) == 0) best[t / DCA_WAVE] = key;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < GR_WAVES; ++w) key = best[w] > key ? best[w] : key;
    if (key)
      __hip_atomic_fetch_max((unsigned long long*)(ws + (long)b * DCA_GROUND_WS_LEN), key, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct GrFit {
  int r_lo, r_hi, min_votes, min_inliers;
  float tol;
};

// ---- 3. the sums of round `round`: grid (<= GR_MAX_BLOCKS, B) ------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void gp_sums_kernel(GrFrame f, GrFit g, const double* plane, long long* ws, int round) {
  __shared__ long long part[GR_WAVES][GM_SUMS];
  const int t = threadIdx.x, b = blockIdx.y;
  long long* w = ws + (long)b * DCA_GROUND_WS_LEN;
  int d_top = 0, d_bot = 0;
  float a32 = 0.f, b32 = 0.f, c32 = 0.f;
  if (round == 0) {
    int vote;
    gm_hough_unkey(coherent_load64(w), f.NB, &vote, &d_top, &d_bot);
    if (vote < g.min_votes) return;                          // status 1 (the whole workgroup: the key is one word)
  } else {
    const double* P = plane + (long)b * DCA_GROUND_PLANE_LEN;
    if (coherent_loadd(P + 5) != 0.0) return;                // status 1 or 2: the remaining rounds do nothing
    a32 = (float)coherent_loadd(P + 0), b32 = (float)coherent_loadd(P + 1), c32 = (float)coherent_loadd(P + 2);
  }
  const int uc = f.cols / 2, vc = f.rows / 2;
  const long n = (long)(g.r_hi - g.r_lo) * f.cols;
  long long S[GM_SUMS];
#pragma unroll
  for (int k = 0; k < GM_SUMS; ++k) S[k] = 0;
  for (long i = (long)blockIdx.x * GR_THREADS + t; i < n; i += (long)gridDim.x * GR_THREADS) {
    const int rr = (int)(i / f.cols), c = (int)(i - (long)rr * f.cols), r = g.r_lo + rr;
    float d;
    int q;
    if (!f.valid(f.at(b, r, c), d, q)) continue;
    const float p = round == 0 ? gm_line_disp(d_top, d_bot, r, f.rows) : gm_plane_disp(a32, b32, c32, c - uc, r - vc);
    if (!(fabsf(d - p) <= g.tol)) continue;
    const long long u = c - uc, v = r - vc, qq = q;
    S[GM_N] += 1, S[GM_SU] += u, S[GM_SV] += v, S[GM_SQ] += qq;
    S[GM_SUU] += u * u, S[GM_SUV] += u * v, S[GM_SVV] += v * v;
    S[GM_SUQ] += u * qq, S[GM_SVQ] += v * qq, S[GM_SQQ] += qq * qq;
  }
#pragma unroll
  for (int k = 0; k < GM_SUMS; ++k) {
#pragma unroll
    for (int o = DCA_WAVE / 2; o > 0; o >>= 1) S[k] += __shfl_xor(S[k], o, DCA_WAVE);
    if ((t & (DCA_WAVE - 1)) == 0) part[t / DCA_WAVE][k] = S[k];
  }
  __syncthreads();
  if (t < GM_SUMS) {
    long long s = 0;
#pragma unroll
    for (int v = 0; v < GR_WAVES; ++v) s += part[v][t];
    if (s != 0)
      __hip_atomic_fetch_add((unsigned long long*)(w + 8 + GM_SUMS * round + t), (unsigned long long)s, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct GrCalib {
  int calibrated;
  double f, baseline, cx, cy, doffs, v0;
};

// ---- 4. the record after round `round` (-1: refine = 0, the Hough line alone): grid (B), one thread works -----------------------
__global__ __launch_bounds__(DCA_WAVE) void gp_solve_kernel(double* plane, const long long* ws, int rows, int cols, int NB,
                                                            GrFit g, GrCalib k, int round) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  const long long* w = ws + (long)b * DCA_GROUND_WS_LEN;
  double* P = plane + (long)b * DCA_GROUND_PLANE_LEN;
  double rec[DCA_GROUND_PLANE_LEN];
  if (round <= 0) {
    int vote, d_top, d_bot;
    gm_hough_unkey(coherent_load64(w), NB, &vote, &d_top, &d_bot);
#pragma unroll
    for (int i = 0; i < DCA_GROUND_PLANE_LEN; ++i) rec[i] = 0.0;
    gm_line_plane(d_top, d_bot, rows, &rec[1], &rec[2]);
    rec[5] = vote < g.min_votes ? 1.0 : 0.0;
    rec[6] = (double)d_top, rec[7] = (double)d_bot, rec[8] = (double)vote;
    rec[13] = (double)(cols / 2), rec[14] = (double)(rows / 2);
  } else {
#pragma unroll
    for (int i = 0; i < DCA_GROUND_PLANE_LEN; ++i) rec[i] = coherent_loadd(P + i);
  }
  if (round >= 0 && rec[5] == 0.0) {
    long long S[GM_SUMS];
#pragma unroll
    for (int i = 0; i < GM_SUMS; ++i) S[i] = (long long)coherent_load64(w + 8 + GM_SUMS * round + i);
    double fit[4];
    const bool solved = gm_solve(S, fit);
    const bool ok = solved && S[GM_N] >= g.min_inliers;       // selects, no branch: the record keeps the last good plane
    rec[0] = ok ? fit[0] : rec[0], rec[1] = ok ? fit[1] : rec[1], rec[2] = ok ? fit[2] : rec[2];
    rec[3] = ok ? (double)S[GM_N] : rec[3], rec[4] = ok ? fit[3] : rec[4];
    rec[5] = ok ? 0.0 : 2.0;
    rec[15] = ok ? (double)(round + 1) : rec[15];
  }
  if (k.calibrated)
    gm_pose(rec[0], rec[1], rec[2], rec[13], rec[14], k.f, k.baseline, k.cx, k.cy, k.doffs, k.v0, &rec[9]);
#pragma unroll
  for (int i = 0; i < DCA_GROUND_PLANE_LEN; ++i) P[i] = rec[i];
}

// ---- the segmentation --------------------------------------------------------------------------------------------------------
struct GsArgs {
  const double* plane;
  float tol_d, h_ground, h_max, f, fb, cx, doffs, x_min, inv_cell, max_depth;
  int NX, NZ, min_run;
};

struct GsPlane {
  float a, b, c, hs;
  bool ok;
};

__device__ __forceinline__ GsPlane gs_plane(const double* plane, int b) {
  const double* P = plane + (long)b * DCA_GROUND_PLANE_LEN;
  GsPlane p;
  p.a = (float)coherent_loadd(P + 0), p.b = (float)coherent_loadd(P + 1), p.c = (float)coherent_loadd(P + 2);
  p.hs = (float)coherent_loadd(P + 9);
  p.ok = coherent_loadd(P + 5) != 1.0 && p.hs > 0.f;
  return p;
}

// THE label of window pixel (r, c), with its disparity and its height (0 where the label is 0)
__device__ __forceinline__ int gs_label(const GrFrame& f, const GsArgs& s, const GsPlane& P, int b, int r, int c, float& d,
                                        float& den, float& h) {
  int q;
  h = 0.f;
  den = 0.f;
  const bool valid = f.valid(f.at(b, r, c), d, q);
  if (!P.ok || !valid) return 0;
  den = d + s.doffs;
  if (!(den > 0.f)) return 0;
  const float p = gm_plane_disp(P.a, P.b, P.c, c - f.cols / 2, r - f.rows / 2);
  const float pden = p + s.doffs;
  h = (P.hs * (den - pden)) / den;
  if (fabsf(d - p) <= s.tol_d || fabsf(h) <= s.h_ground) return 1;
  if (h < 0.f) return 4;
  if (h > s.h_max) return 3;
  return 2;
}

// grid (ceil(cols / DCA_WAVE), B), one wave per workgroup
__global__ __launch_bounds__(DCA_WAVE) void gs_column_kernel(GrFrame f, GsArgs s, int* __restrict__ free_row,
                                                             float* __restrict__ free_disp, int* __restrict__ bev) {
  const int t = threadIdx.x, b = blockIdx.y;
  if (bev) {
    const long cells = 2L * s.NZ * s.NX;
    int* g = bev + (long)b * cells;
    for (long k = (long)blockIdx.x * DCA_WAVE + t; k < cells; k += (long)gridDim.x * DCA_WAVE) g[k] = 0;
  }
  const int c = blockIdx.x * DCA_WAVE + t;
  if (!free_row || c >= f.cols) return;
  const GsPlane P = gs_plane(s.plane, b);
  int run = 0, start = -1, row = -1;
  float dstart = 0.f, disp = 0.f;
  for (int r = f.rows - 1; r >= 0; --r) {
    float d, den, h;
    if (gs_label(f, s, P, b, r, c, d, den, h) == 2) {
      if (run == 0) start = r, dstart = d;
      if (++run == s.min_run) {
        row = start, disp = dstart;
        break;
      }
    } else {
      run = 0;
    }
  }
  free_row[(long)b * f.cols + c] = row;
  free_disp[(long)b * f.cols + c] = disp;
}

// grid (ceil(rows cols / GR_THREADS), B)
__global__ __launch_bounds__(GR_THREADS) void gs_pixel_kernel(GrFrame f, GsArgs s, unsigned char* __restrict__ label,
                                                              float* __restrict__ height, int* bev) {
  const int n = f.rows * f.cols, b = blockIdx.y, lane = threadIdx.x & (DCA_WAVE - 1);
  const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
  const GsPlane P = gs_plane(s.plane, b);
  int lab = 0, cell = -1;
  if (i < n) {
    const int r = (int)(i / f.cols), c = (int)(i - (long)r * f.cols);
    float d, den, h;
    lab = gs_label(f, s, P, b, r, c, d, den, h);
    if (label) label[(long)b * n + i] = (unsigned char)lab;
    if (height) height[(long)b * n + i] = h;
    if (bev && (lab == 1 || lab == 2)) {
      const float Z = s.fb / den;
      const float X = (((float)c - s.cx) * Z) / s.f;
      const float fx = floorf((X - s.x_min) * s.inv_cell), fz = floorf(Z * s.inv_cell);
      if (fx >= 0.f && fx < (float)s.NX && fz >= 0.f && fz < (float)s.NZ && Z <= s.max_depth)
        cell = ((lab - 1) * s.NZ + (int)fz) * s.NX + (int)fx;
    }
  }
  if (!bev) return;
  // every lane of the wave is here: a lane leads the run of consecutive lanes with its cell and adds the run's length
  const int prev = __shfl_up(cell, 1, DCA_WAVE);
  const bool leader = lane == 0 || prev != cell;
  const unsigned long long leaders = __ballot(leader);
  if (leader && cell >= 0) {
    const unsigned long long above = lane == DCA_WAVE - 1 ? 0ull : leaders & ~((2ull << lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : DCA_WAVE;
    __hip_atomic_fetch_add(bev + (long)b * 2 * s.NZ * s.NX + cell, next - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }
inline bool finite_d(double v) { return fabs(v) < (double)INFINITY; }

inline bool gr_frame_ok(const float* d, const float* mask, int B, int Hc, int Wc, int y0, int rows, int cols, int NB,
                        float min_disp, float mask_min) {
  return d && B > 0 && B <= 65535 && dca_window_ok(Hc, Wc, y0, rows, cols) && rows <= DCA_GROUND_MAX_DIM &&
         cols <= DCA_GROUND_MAX_DIM && NB >= 8 && NB <= DCA_GROUND_MAX_DISP && min_disp >= 0.f && finite_f(min_disp) &&
         !(mask && mask_min != mask_min);
}

}  // namespace

extern "C" int dca_ground_plane(const float* d, const float* mask, double* plane, int* vdisp, long long* ws, int B, int Hc,
                                int Wc, int y0, int rows, int cols, int max_disp, int r_lo, int r_hi, int min_rise,
                                int min_votes, int refine, int min_inliers, float min_disp, float tol, float mask_min,
                                int calibrated, double f, double baseline, double cx, double cy, double doffs, double v0,
                                hipStream_t stream) {
  DCA_REQUIRE(gr_frame_ok(d, mask, B, Hc, Wc, y0, rows, cols, max_disp, min_disp, mask_min));
  DCA_REQUIRE(plane && vdisp && ws && ((uintptr_t)plane & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)vdisp & 3) == 0);
  DCA_REQUIRE(rows >= 2 && r_lo >= 0 && r_lo < r_hi && r_hi <= rows);
  DCA_REQUIRE(min_rise >= 1 && min_rise <= max_disp && min_votes >= 1 && refine >= 0 && refine <= DCA_GROUND_MAX_REFINE);
  DCA_REQUIRE(min_inliers >= 3 && tol >= 0.f && finite_f(tol));
  DCA_REQUIRE(calibrated == 0 || calibrated == 1);
  if (calibrated) {
    DCA_REQUIRE(f > 0.0 && finite_d(f) && baseline > 0.0 && finite_d(baseline));
    DCA_REQUIRE(finite_d(cx) && finite_d(cy) && finite_d(doffs) && finite_d(v0));
  }
  const int NB = max_disp;
  const GrFrame fr = {d, mask, Hc, Wc, y0, rows, cols, NB, min_disp, mask_min};
  const GrFit g = {r_lo, r_hi, min_votes, min_inliers, tol};
  const GrCalib k = {calibrated, f, baseline, cx, cy, doffs, v0};
  const int ncand = (NB - 1) * 2 * NB;
  hipLaunchKernelGGL(gp_vdisp_kernel, dim3((unsigned)cdiv(rows, GR_WAVES), (unsigned)B), dim3(GR_THREADS), 0, stream, fr, vdisp,
                     ws);
  hipLaunchKernelGGL(gp_vote_kernel, dim3((unsigned)cdiv(ncand, GR_THREADS), (unsigned)B), dim3(GR_THREADS), 0, stream,
                     (const int*)vdisp, ws, rows, NB, r_lo, r_hi, min_rise, ncand);
  int blocks = cdiv((long)(r_hi - r_lo) * cols, GR_THREADS);
  blocks = blocks > GR_MAX_BLOCKS ? GR_MAX_BLOCKS : blocks;
  for (int round = 0; round < refine; ++round) {
    hipLaunchKernelGGL(gp_sums_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(GR_THREADS), 0, stream, fr, g,
                       (const double*)plane, ws, round);
    hipLaunchKernelGGL(gp_solve_kernel, dim3((unsigned)B), dim3(DCA_WAVE), 0, stream, plane, (const long long*)ws, rows, cols,
                       NB, g, k, round);
  }
  if (refine == 0)
    hipLaunchKernelGGL(gp_solve_kernel, dim3((unsigned)B), dim3(DCA_WAVE), 0, stream, plane, (const long long*)ws, rows, cols,
                       NB, g, k, -1);
  return dca_launch_status();
}

extern "C" int dca_ground_segment(const float* d, const float* mask, const double* plane, unsigned char* label, float* height,
                                  int* free_row, float* free_disp, int* bev, int B, int Hc, int Wc, int y0, int rows, int cols,
                                  int max_disp, float min_disp, float mask_min, float tol_d, float h_ground, float h_max,
                                  int min_run, float f, float fb, float cx, float doffs, float x_min, float inv_cell,
                                  float max_depth, int NX, int NZ, hipStream_t stream) {
  DCA_REQUIRE(gr_frame_ok(d, mask, B, Hc, Wc, y0, rows, cols, max_disp, min_disp, mask_min));
  DCA_REQUIRE(plane && ((uintptr_t)plane & 7) == 0 && (label || height || free_row || bev));
  DCA_REQUIRE((free_row == nullptr) == (free_disp == nullptr));
  DCA_REQUIRE(tol_d >= 0.f && finite_f(tol_d) && h_ground >= 0.f && finite_f(h_ground) && finite_f(h_max) && min_run >= 1);
  DCA_REQUIRE(f > 0.f && finite_f(f) && fb > 0.f && finite_f(fb) && finite_f(cx) && finite_f(doffs) && finite_f(x_min));
  if (bev) {
    DCA_REQUIRE(inv_cell > 0.f && finite_f(inv_cell) && max_depth > 0.f && finite_f(max_depth));
    DCA_REQUIRE(NX >= 1 && NZ >= 1 && 2L * NX * NZ < (1L << 31) && ((uintptr_t)bev & 3) == 0);
  }
  const GrFrame fr = {d, mask, Hc, Wc, y0, rows, cols, max_disp, min_disp, mask_min};
  const GsArgs s = {plane, tol_d, h_ground, h_max, f, fb, cx, doffs, x_min, inv_cell, max_depth, NX, NZ, min_run};
  if (free_row || bev)
    hipLaunchKernelGGL(gs_column_kernel, dim3((unsigned)cdiv(cols, DCA_WAVE), (unsigned)B), dim3(DCA_WAVE), 0, stream, fr, s,
                       free_row, free_disp, bev);
  if (label || height || bev)
    hipLaunchKernelGGL(gs_pixel_kernel, dim3((unsigned)cdiv((long)rows * cols, GR_THREADS), (unsigned)B), dim3(GR_THREADS), 0,
                       stream, fr, s, label, height, bev);
  return dca_launch_status();
}
