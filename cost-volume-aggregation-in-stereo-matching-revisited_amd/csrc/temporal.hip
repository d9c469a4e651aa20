// Temporal stereo (nothing in the reference computes it): the previous frame's disparity state warped
// by the known ego-motion into the current left image, and its per-pixel fusion with the current measurement -- the
// definitions of include/dca_hip.h (dca_disp_reproject, dca_temporal_fuse) as they are written; the arithmetic is
// temporal_math.h's, shared with the host check.
//
// dca_disp_reproject, three launches:
//  1. clear:   the workspace of H W 64-bit keys becomes 0, the two counters 0;
//  2. scatter: one thread per SOURCE pixel projects it by G and, if it is kept, takes the agent-scope, relaxed 64-bit INTEGER
//              fetch_max of  bits(den') << 32 | (0xFFFFFFFF - source index)  into the target's word.  den' >= 0, so its bits
//              order as the floats do: the nearest surface wins, among equal den' the smallest source index, whatever the
//              order of arrival.  No float atomics; bitwise reproducible;
//  3. resolve: a workgroup stages the HIGH words of a TP_TW x TP_TH tile with its halo in LDS, takes the window maximum along
//              rows, then along columns (as the LiDAR resolve takes its minimum), tests the winner against it and gathers
//              the payload from the winning source pixel; eight workgroups per CU walk the tiles.
// dca_disp_reproject_dev: the same three launches with the matrix read from device memory (a pose estimated there, odometry.hip).
// dca_temporal_fuse: one launch, one thread per pixel.
// The two counters take integer atomicAdds, one per workgroup.  Kernel boundaries are the only global synchronisation; the
// keys, written by another kernel's atomics, are read with agent-scope loads.  ~40 B per pixel over
// maps that fit in L2: the launches are latency-bound, the kernels are kept plain.
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "temporal_math.h"

// the formulas of include/dca_hip.h as they are written: every operation rounded on its own, no contraction into fma
#pragma clang fp contract(off)

namespace {

#define TP_THREADS 256
#define TP_TW 32
#define TP_TH 8
#define TP_R DCA_TEMPORAL_MAX_RADIUS
#define TP_HALO_A ((TP_TH + 2 * TP_R + TP_TH - 1) / TP_TH)
#define TP_HALO_B ((TP_TW + 2 * TP_R + TP_TW - 1) / TP_TW)
static_assert(TP_TW * TP_TH == TP_THREADS && TP_THREADS % DCA_WAVE == 0, "one thread per tile pixel, whole waves");

__device__ __forceinline__ unsigned long long coherent_load64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the wave totals of a workgroup (a ballot's population count: the same number in every lane) -> ONE integer atomicAdd.
// Every thread of the workgroup must call it.
__device__ __forceinline__ void block_add(unsigned long long* counter, unsigned wave_total) {
  __shared__ unsigned totals[TP_THREADS / DCA_WAVE];
  if ((threadIdx.x & (DCA_WAVE - 1)) == 0) totals[threadIdx.x / DCA_WAVE] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < TP_THREADS / DCA_WAVE; ++w) sum += totals[w];
    if (sum) atomicAdd(counter, (unsigned long long)sum);
  }
}

__global__ __launch_bounds__(TP_THREADS) void tp_clear_kernel(unsigned long long* __restrict__ ws, long hw,
                                                              unsigned long long* __restrict__ count) {
  for (long i = (long)blockIdx.x * TP_THREADS + threadIdx.x; i < hw; i += (long)gridDim.x * TP_THREADS) ws[i] = 0ull;
  if (count && blockIdx.x == 0 && threadIdx.x < 2) count[threadIdx.x] = 0ull;
}

// DEV: the matrix is read from device memory (another kernel wrote it: agent-scope loads), the rest of `p` is by value
template <bool DEV>
__device__ __forceinline__ void tp_load_g(TmProj& p, const float* g) {
  if (DEV) {
#pragma unroll
    for (int i = 0; i < 12; ++i) p.g[i] = dca_coherent_loadf(g + i);
  }
}

template <bool DEV>
__global__ __launch_bounds__(TP_THREADS) void tp_scatter_kernel(const float* __restrict__ disp, const float* __restrict__ mask,
                                                                float mask_min, TmProj p, const float* g, unsigned long long* ws,
                                                                unsigned long long* __restrict__ count) {
  tp_load_g<DEV>(p, g);
  const long hw = (long)p.H * p.W;
  const long i = (long)blockIdx.x * TP_THREADS + threadIdx.x;
  bool keep = false;
  if (i < hw) {
    const int v = (int)(i / p.W), u = (int)(i - (long)v * p.W);
    const float d = disp[i];
    const bool pass = mask ? mask[i] >= mask_min : true;
    long target = 0;
    float denp = 0.f;
    keep = tm_project(p, u, v, d, &target, &denp) && pass;
    // tm_project has checked 0 <= target < H W in float before the conversion
    if (keep) __hip_atomic_fetch_max(ws + target, tm_key(denp, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (count) block_add(count + 1, (unsigned)__popcll(__ballot(keep)));
}

struct TpOut {
  float* pred;
  float* pred_var;
  unsigned char* pred_age;
  float* hints;
  unsigned long long* count;
  float occl_px, q;
  int hint_min_age;
};

// persistent: a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... and adds its count once at the end
template <bool DEV>
__global__ __launch_bounds__(TP_THREADS) void tp_resolve_kernel(const unsigned long long* ws, const float* __restrict__ disp,
                                                                const float* __restrict__ var,
                                                                const unsigned char* __restrict__ age, TmProj p, const float* g,
                                                                int tiles_x, int tiles, int rx, int ry, TpOut o) {
  tp_load_g<DEV>(p, g);
  __shared__ unsigned tile[TP_TH + 2 * TP_R][TP_TW + 2 * TP_R];      // the high words of the tile with its halo; 0 outside the image
  __shared__ unsigned rowmax[TP_TH + 2 * TP_R][TP_TW];               // maximum over columns c-rx .. c+rx of every halo row
  const int H = p.H, W = p.W;
  const int t = threadIdx.x;
  const int hh = TP_TH + 2 * ry, hw = TP_TW + 2 * rx;               // rx, ry <= TP_R: inside the arrays
  const int lr = t / TP_TW, lc = t - lr * TP_TW;
  unsigned written = 0;                                             // of this wave, over all its tiles
  for (int id = blockIdx.x; id < tiles; id += gridDim.x) {
    const int ty0 = (id / tiles_x) * TP_TH, tx0 = (id % tiles_x) * TP_TW;
    unsigned halo[TP_HALO_A][TP_HALO_B];
#pragma unroll
    for (int a = 0; a < TP_HALO_A; ++a) {
#pragma unroll
      for (int b = 0; b < TP_HALO_B; ++b) {
        const int hr = lr + a * TP_TH, hc = lc + b * TP_TW;
        const int r = ty0 - ry + hr, c = tx0 - rx + hc;
        halo[a][b] = (hr < hh && hc < hw && r >= 0 && r < H && c >= 0 && c < W)
                         ? (unsigned)(coherent_load64(ws + ((long)r * W + c)) >> 32)
                         : 0u;
      }
    }
#pragma unroll
    for (int a = 0; a < TP_HALO_A; ++a) {
#pragma unroll
      for (int b = 0; b < TP_HALO_B; ++b) {
        const int hr = lr + a * TP_TH, hc = lc + b * TP_TW;
        if (hr < hh && hc < hw) tile[hr][hc] = halo[a][b];
      }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < TP_HALO_A; ++a) {
      const int hr = lr + a * TP_TH;
      if (hr < hh) {
        unsigned m = tile[hr][lc];
        for (int k = 1; k <= 2 * rx; ++k) m = max(m, tile[hr][lc + k]);
        rowmax[hr][lc] = m;
      }
    }
    __syncthreads();
    unsigned m = rowmax[lr][lc];
    for (int k = 1; k <= 2 * ry; ++k) m = max(m, rowmax[lr + k][lc]);
    const int r = ty0 + lr, c = tx0 + lc;
    const bool inside = r < H && c < W;
    const long at = (long)r * W + c;
    const unsigned long long key = inside ? coherent_load64(ws + at) : 0ull;
    const float denp = tm_key_den(key);
    const bool visible = key != 0ull && tm_visible(denp, o.occl_px, tm_float(m));
    if (inside) {
      float d = 0.f, v = 0.f;
      unsigned char a = 0;
      if (visible) {
        const long src = tm_key_src(key);                           // a kept source pixel: 0 <= src < H W
        const int sv = (int)(src / W), su = (int)(src - (long)sv * W);
        const float z = tm_ratio(p, su, sv, disp[src]);
        d = denp - p.doffs;
        v = tm_pred_var(var[src], z, o.q);
        a = tm_pred_age(age[src]);
      }
      if (o.pred) o.pred[at] = d;
      if (o.pred_var) o.pred_var[at] = v;
      if (o.pred_age) o.pred_age[at] = a;
      if (o.hints) o.hints[at] = (visible && (int)a >= o.hint_min_age) ? d : 0.f;
    }
    written += (unsigned)__popcll(__ballot(visible));
    __syncthreads();                                                // tile and rowmax are rewritten by the next tile
  }
  if (o.count) block_add(o.count, written);
}

struct TfArgs {
  const float* pred;
  const float* pred_var;
  const unsigned char* pred_age;
  const float* meas;
  const float* mask;
  const float* meas_var_map;
  float* disp;
  float* var;
  unsigned char* age;
  float* innov;
  int Wc, y0, rows, cols;
  float meas_var, min_disp, mask_min, gate2, var_max;
};

// no __restrict__: the new state may lie over the prediction (every thread reads its pixel before it writes it)
__global__ __launch_bounds__(TP_THREADS) void tp_fuse_kernel(TfArgs a) {
  const long n = (long)a.rows * a.cols;
  const long i = (long)blockIdx.x * TP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int r = (int)(i / a.cols), c = (int)(i - (long)r * a.cols);
  const long at = (long)(a.y0 + r) * a.Wc + c;                      // in the measurement's frame
  const float m = a.meas[at];
  const float vm = a.meas_var_map ? a.meas_var_map[at] : a.meas_var;
  const bool pass = a.mask ? a.mask[at] >= a.mask_min : true;
  const bool m_ok = tm_meas_ok(m, vm, a.min_disp) && pass;
  float pred = 0.f, pv = 0.f;
  unsigned char pa = 0;
  if (a.pred) {
    pred = a.pred[i];
    pv = a.pred_var[i];
    pa = a.pred_age[i];
  }
  const bool p_ok = a.pred != nullptr && tm_pred_ok(pred, pv, a.var_max);
  const TmState s = tm_fuse(m_ok, m, vm, p_ok, pred, pv, pa, a.gate2);
  if (a.disp) a.disp[i] = s.disp;
  if (a.var) a.var[i] = s.var;
  if (a.age) a.age[i] = s.age;
  if (a.innov) a.innov[i] = s.innov;
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }

// the launches of both entry points: g_dev NULL -> the matrix of `p`, else the twelve floats at g_dev
template <bool DEV>
int tp_reproject(const float* disp, const float* var, const unsigned char* age, const float* mask, float mask_min, const TmProj& p,
                 const float* g_dev, int rx, int ry, float occl_px, float q, int hint_min_age, float* pred, float* pred_var,
                 unsigned char* pred_age, float* hints, long long* count, long long* workspace, hipStream_t stream) {
  const int H = p.H, W = p.W;
  const float doffs = p.doffs, min_disp = p.min_disp, max_disp = p.max_disp, min_ratio = p.min_ratio;
  DCA_REQUIRE(disp && var && age);
  DCA_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31));
  DCA_REQUIRE(rx >= 0 && rx <= DCA_TEMPORAL_MAX_RADIUS && ry >= 0 && ry <= DCA_TEMPORAL_MAX_RADIUS);
  DCA_REQUIRE(occl_px >= 0.f && finite_f(occl_px) && q >= 0.f && finite_f(q) && min_ratio >= 0.f && finite_f(min_ratio));
  DCA_REQUIRE(doffs >= 0.f && finite_f(doffs) && min_disp >= 0.f && finite_f(min_disp) && finite_f(max_disp) &&
              max_disp >= min_disp);
  DCA_REQUIRE(hint_min_age >= 0 && hint_min_age <= 255);
  DCA_REQUIRE(!mask || mask_min == mask_min);
  DCA_REQUIRE(pred || pred_var || pred_age || hints || count);
  DCA_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)count & 7) == 0);
  if (DEV) {
    DCA_REQUIRE(g_dev && ((uintptr_t)g_dev & 3) == 0);
  } else {
    for (int i = 0; i < 12; ++i) DCA_REQUIRE(finite_f(p.g[i]));
  }
  const TpOut o = {pred, pred_var, pred_age, hints, (unsigned long long*)count, occl_px, q, hint_min_age};
  unsigned long long* ws = (unsigned long long*)workspace;
  const long hw = (long)H * W;
  const long per_px = (hw + TP_THREADS - 1) / TP_THREADS;
  const long clear = per_px > 2048 ? 2048 : per_px;
  const int tiles_x = cdiv(W, TP_TW);
  const long tiles = (long)tiles_x * cdiv(H, TP_TH);
  hipLaunchKernelGGL(tp_clear_kernel, dim3((unsigned)clear), dim3(TP_THREADS), 0, stream, ws, hw, o.count);
  hipLaunchKernelGGL(tp_scatter_kernel<DEV>, dim3((unsigned)per_px), dim3(TP_THREADS), 0, stream, disp, mask, mask_min, p, g_dev,
                     ws, o.count);
  const long resolve = tiles < 8L * dca_num_cus() ? tiles : 8L * dca_num_cus();      // 8 x 4 waves: what a CU holds
  hipLaunchKernelGGL(tp_resolve_kernel<DEV>, dim3((unsigned)resolve), dim3(TP_THREADS), 0, stream, (const unsigned long long*)ws,
                     disp, var, age, p, g_dev, tiles_x, (int)tiles, rx, ry, o);
  return dca_launch_status();
}

}  // namespace

extern "C" int dca_disp_reproject(const float* disp, const float* var, const unsigned char* age, const float* mask,
                                  float mask_min, float g00, float g01, float g02, float g03, float g10, float g11, float g12,
                                  float g13, float g20, float g21, float g22, float g23, int H, int W, float doffs,
                                  float min_disp, float max_disp, float min_ratio, int rx, int ry, float occl_px, float q,
                                  int hint_min_age, float* pred, float* pred_var, unsigned char* pred_age, float* hints,
                                  long long* count, long long* workspace, hipStream_t stream) {
  const TmProj p = {{g00, g01, g02, g03, g10, g11, g12, g13, g20, g21, g22, g23}, doffs, min_disp, max_disp, min_ratio, H, W};
  return tp_reproject<false>(disp, var, age, mask, mask_min, p, nullptr, rx, ry, occl_px, q, hint_min_age, pred, pred_var, pred_age,
                             hints, count, workspace, stream);
}

extern "C" int dca_disp_reproject_dev(const float* disp, const float* var, const unsigned char* age, const float* mask,
                                      float mask_min, const float* g, int H, int W, float doffs, float min_disp, float max_disp,
                                      float min_ratio, int rx, int ry, float occl_px, float q, int hint_min_age, float* pred,
                                      float* pred_var, unsigned char* pred_age, float* hints, long long* count,
                                      long long* workspace, hipStream_t stream) {
  const TmProj p = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, doffs, min_disp, max_disp, min_ratio, H, W};
  return tp_reproject<true>(disp, var, age, mask, mask_min, p, g, rx, ry, occl_px, q, hint_min_age, pred, pred_var, pred_age, hints,
                            count, workspace, stream);
}

extern "C" int dca_temporal_fuse(const float* pred, const float* pred_var, const unsigned char* pred_age, const float* meas,
                                 const float* mask, const float* meas_var_map, float meas_var, float* disp, float* var,
                                 unsigned char* age, float* innov, int Hc, int Wc, int y0, int rows, int cols, float min_disp,
                                 float mask_min, float gate2, float var_max, hipStream_t stream) {
  DCA_REQUIRE(meas && (disp || var || age || innov));
  DCA_REQUIRE(!pred || (pred_var && pred_age));
  DCA_REQUIRE(dca_window_ok(Hc, Wc, y0, rows, cols));
  DCA_REQUIRE(meas_var_map || (meas_var > 0.f && finite_f(meas_var)));
  DCA_REQUIRE(min_disp >= 0.f && finite_f(min_disp));
  DCA_REQUIRE(gate2 >= 0.f && var_max >= 0.f);                      // (a NaN fails both; +inf switches either off)
  DCA_REQUIRE(!mask || mask_min == mask_min);
  const TfArgs a = {pred, pred_var, pred_age, meas, mask, meas_var_map, disp, var, age, innov, Wc, y0, rows, cols,
                    meas_var, min_disp, mask_min, gate2, var_max};
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(tp_fuse_kernel, dim3((unsigned)((n + TP_THREADS - 1) / TP_THREADS)), dim3(TP_THREADS), 0, stream, a);
  return dca_launch_status();
}
