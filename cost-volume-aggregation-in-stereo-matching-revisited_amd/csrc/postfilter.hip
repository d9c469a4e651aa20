// Disparity post-filter (nothing in the reference computes it): the speckle filter -- connected
// components of similar disparity, the small ones dropped -- and a small median, the definitions of include/dca_hip.h
// (dca_speckle_filter, dca_median_filter) as they are written.
//
// Speckle filter, four launches, the kernel boundaries being the only global synchronisation:
//  1. local:  one workgroup per DCA_SPK_TILE_H x DCA_SPK_TILE_W tile.  Horizontal runs by pointer jumping (log2 TW rounds,
//             no atomics), then the vertical joins by union-find with LDS atomicMin, one union per pair of runs that meet
//             rather than one per pixel.  label = the window index of the tile-local root (-1: inactive), count = the
//             tile-local component size at that root, 0 everywhere else.  Every word of both buffers is written: a call
//             re-initialises its workspace itself.
//  2. merge:  one thread per pixel pair across a tile edge (spk_merge_edge, spk_unionfind.h), union-find in global memory.
//             Workgroups on different XCDs read and write the same labels here: every label access of this launch is an
//             agent-scope atomic (a plain load may be served from a stale L2 line of the thread's own XCD).
//  3. count:  a tile-local root whose global root is another pixel adds its count there: ONE integer atomic per (tile,
//             local component), never one per pixel -- a frame that is one component sends a few hundred adds to one word,
//             not rows x cols.  The root is written back into the local root's label, so launch 4 walks two links.
//  4. apply:  pixel -> tile-local root -> global root, its count, the outputs.
// Everything after the comparison |a - b| <= max_diff is integer arithmetic or a copy: the outputs do not depend on the
// order in which anything above happens.  The invariants (labels only decrease, label[x] <= x, no loop waits for another
// workgroup) are written down with the union-find itself, spk_unionfind.h.
//
// Median: ONE launch, the tile with its halo as order keys in LDS; the candidate of rank (n-1)/2 is found by counting
// (n <= 25: n^2 comparisons in registers, no sorting network per n).
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "spk_unionfind.h"

// the comparison of include/dca_hip.h as it is written: the subtraction rounded on its own
#pragma clang fp contract(off)

namespace {

#define PF_THREADS 256
#define PF_TH DCA_SPK_TILE_H
#define PF_TW DCA_SPK_TILE_W
#define PF_PIX (PF_TH * PF_TW)
#define PF_PER (PF_PIX / PF_THREADS)
static_assert(PF_PIX % PF_THREADS == 0 && PF_THREADS % PF_TW == 0, "whole tile rows per pass of the workgroup");
static_assert((PF_TW & (PF_TW - 1)) == 0 && PF_TW <= 64, "PF_JUMPS rounds of pointer jumping cover a tile row");
#define PF_JUMPS 6                                           // 2^6 >= PF_TW

// ONE batch of frames (B,Hc,Wc) with the window rows x cols at frame row y0, column 0 of every image
struct PfFrame {
  const float* d;
  const float* mask;                                         // indexed like d, or NULL
  int Hc, Wc, y0, rows, cols;
  float mask_min;
  __device__ __forceinline__ long at(int b, int r, int c) const { return ((long)b * Hc + (y0 + r)) * (long)Wc + c; }
  __device__ __forceinline__ bool active(float v, long i) const { return spk_finite(v) && (!mask || mask[i] >= mask_min); }
};

struct LdsLabels {                                           // the labels of one tile, shared by one workgroup
  int* l;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(l + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void store(int i, int v) const { __hip_atomic_store(l + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(l + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct GlobalLabels {                                        // the labels of one image, shared by workgroups on every XCD
  int* l;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(l + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(int i, int v) const { __hip_atomic_store(l + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(l + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct WindowValues {                                        // the disparities of one image's window
  const float* d;
  int Wc;
  __device__ __forceinline__ float at(int r, int c) const { return d[(long)r * Wc + c]; }
};

// grid (tiles, B)
__global__ __launch_bounds__(PF_THREADS) void spk_local_kernel(PfFrame f, float max_diff, int tiles_x, int* __restrict__ label,
                                                               int* __restrict__ count) {
  __shared__ float val[PF_PIX];
  __shared__ int lab[PF_PIX];
  __shared__ int cnt[PF_PIX];
  __shared__ unsigned char join[PF_PIX];                     // bit 0: joined with the left neighbour, bit 1: with the upper one
  const int t = threadIdx.x, b = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * PF_TH, tx0 = (blockIdx.x % tiles_x) * PF_TW;
  const LdsLabels L = {lab};
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS, r = ty0 + i / PF_TW, c = tx0 + i % PF_TW;
    float v = 0.f;
    bool act = false;
    if (r < f.rows && c < f.cols) {
      const long at = f.at(b, r, c);
      v = f.d[at];
      act = f.active(v, at);
    }
    val[i] = v;
    lab[i] = act ? i : -1;
    cnt[i] = 0;
  }
  __syncthreads();
  unsigned joins = 0;                                        // two bits per pixel of this thread
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS, lx = i % PF_TW;
    unsigned j = 0;
    if (lab[i] >= 0) {
      if (lx > 0 && lab[i - 1] >= 0 && spk_joined(val[i], val[i - 1], max_diff)) j |= 1u;
      if (i >= PF_TW && lab[i - PF_TW] >= 0 && spk_joined(val[i], val[i - PF_TW], max_diff)) j |= 2u;
    }
    join[i] = (unsigned char)j;
    joins |= j << (2 * k);
  }
  __syncthreads();
  // horizontal runs: link to the left neighbour, then pointer jumping -- after round n every pixel points at least
  // min(2^n, its distance to the run's start) to the left; a racing read sees the old or the new link, both in the run
#pragma unroll
  for (int k = 0; k < PF_PER; ++k)
    if ((joins >> (2 * k)) & 1u) lab[t + k * PF_THREADS] = t + k * PF_THREADS - 1;
  __syncthreads();
  for (int n = 0; n < PF_JUMPS; ++n) {
#pragma unroll
    for (int k = 0; k < PF_PER; ++k) {
      const int i = t + k * PF_THREADS, p = L.load(i);
      if (p >= 0 && p != i) L.store(i, L.load(p));
    }
    __syncthreads();
  }
  // vertical joins: not where the pixel to the left makes the same union (it is in this run, its upper neighbour in the
  // upper one's run): one union per pair of runs that meet
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS;
    const unsigned j = (joins >> (2 * k)) & 3u;
    if ((j & 2u) && !((j & 1u) && (join[i - 1] & 2u) && (join[i - PF_TW] & 1u))) spk_union(L, i, i - PF_TW);
  }
  __syncthreads();
  int root[PF_PER];
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS;
    root[k] = lab[i] >= 0 ? spk_find(L, i) : -1;             // nothing writes the labels any more
    if (root[k] >= 0) atomicAdd(&cnt[root[k]], 1);
  }
  __syncthreads();
  int* lab_g = label + (long)b * f.rows * f.cols;
  int* cnt_g = count + (long)b * f.rows * f.cols;
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS, r = ty0 + i / PF_TW, c = tx0 + i % PF_TW;
    if (r < f.rows && c < f.cols) {
      const int g = r * f.cols + c, rt = root[k];
      // the tile-local order of two pixels is their order by window index: label <= own index holds in the window too
      lab_g[g] = rt >= 0 ? (ty0 + rt / PF_TW) * f.cols + tx0 + rt % PF_TW : -1;
      cnt_g[g] = rt == i ? cnt[i] : 0;
    }
  }
}

// grid (ceil(pairs / PF_THREADS), B)
__global__ __launch_bounds__(PF_THREADS) void spk_merge_kernel(PfFrame f, float max_diff, int tiles_x, int pairs,
                                                               int* label) {
  const int e = blockIdx.x * PF_THREADS + threadIdx.x, b = blockIdx.y;
  if (e >= pairs) return;
  const GlobalLabels G = {label + (long)b * f.rows * f.cols};
  const WindowValues V = {f.d + f.at(b, 0, 0), f.Wc};
  spk_merge_edge<PF_TH, PF_TW>(G, V, e, f.rows, f.cols, tiles_x, max_diff);
}

// grid (ceil(n / PF_THREADS), B), n = rows cols.  The adds go to global roots only, the counts read are those of pixels
// that are not: no word is both read and added to.
__global__ __launch_bounds__(PF_THREADS) void spk_count_kernel(int n, int* label, int* count) {
  const int i = blockIdx.x * PF_THREADS + threadIdx.x;
  if (i >= n) return;
  const GlobalLabels G = {label + (long)blockIdx.y * n};
  int* cnt = count + (long)blockIdx.y * n;
  if (G.load(i) == i) return;                                // a global root keeps its count; an inactive pixel has none
  const int c = cnt[i];
  if (c <= 0) return;                                        // not a tile-local root
  const int r = spk_find(G, i);
  atomicAdd(&cnt[r], c);
  G.store(i, r);                                             // r < i: a label only decreases
}

struct SpkOut {
  float* disp;
  float* valid;
  int* size;
  int max_size;
  float fill;
};

// grid (ceil(n / PF_THREADS), B): the labels and counts are final, plain loads
__global__ __launch_bounds__(PF_THREADS) void spk_apply_kernel(PfFrame f, const int* __restrict__ label,
                                                               const int* __restrict__ count, SpkOut o) {
  const int n = f.rows * f.cols, i = blockIdx.x * PF_THREADS + threadIdx.x, b = blockIdx.y;
  if (i >= n) return;
  const int* lab = label + (long)b * n;
  int size = 0, r = lab[i];
  if (r >= 0) {
    for (int p = lab[r]; p != r; p = lab[r]) r = p;
    size = count[(long)b * n + r];
  }
  const bool keep = size > o.max_size;
  const long at = (long)b * n + i;
  o.valid[at] = keep ? 1.f : 0.f;
  if (o.size) o.size[at] = size;
  if (o.disp) {
    const int row = i / f.cols;
    o.disp[at] = keep ? f.d[f.at(b, row, i - row * f.cols)] : o.fill;
  }
}

#define PF_NONE 0xffffffffu                                   // the key of the bits 0x7fffffff, a NaN: never an active pixel's

// grid (tiles, B); K = 3 or 5
template <int K>
__global__ __launch_bounds__(PF_THREADS) void median_kernel(PfFrame f, int tiles_x, float* __restrict__ out) {
  constexpr int R = K / 2, HW = PF_TW + 2 * R, HH = PF_TH + 2 * R;
  // the order key of every ACTIVE pixel of the tile and its halo, PF_NONE for the others and outside the window: a key
  // that is below no candidate and at or below none (the candidates' keys are smaller), so it is never counted
  __shared__ unsigned key[HH * HW];
  const int t = threadIdx.x, b = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * PF_TH, tx0 = (blockIdx.x % tiles_x) * PF_TW;
  for (int h = t; h < HH * HW; h += PF_THREADS) {
    const int r = ty0 - R + h / HW, c = tx0 - R + h % HW;
    unsigned k = PF_NONE;
    if (r >= 0 && r < f.rows && c >= 0 && c < f.cols) {
      const long at = f.at(b, r, c);
      const float v = f.d[at];
      if (f.active(v, at)) k = spk_key(__float_as_uint(v));
    }
    key[h] = k;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PF_PER; ++k) {
    const int i = t + k * PF_THREADS, ly = i / PF_TW, lx = i % PF_TW, r = ty0 + ly, c = tx0 + lx;
    if (r >= f.rows || c >= f.cols) continue;
    const int h0 = ly * HW + lx;                             // the neighbourhood's top-left corner in the halo tile
    float* dst = out + ((long)b * f.rows + r) * f.cols + c;
    if (key[h0 + R * HW + R] == PF_NONE) {                   // an inactive centre is copied unchanged
      *dst = f.d[f.at(b, r, c)];
      continue;
    }
    unsigned ks[K * K];
    int n = 0;
#pragma unroll
    for (int j = 0; j < K * K; ++j) {
      ks[j] = key[h0 + (j / K) * HW + j % K];
      n += ks[j] != PF_NONE;
    }
    const unsigned tgt = (unsigned)(n - 1) >> 1;             // the centre is a candidate: n >= 1
    unsigned res = ks[R * K + R];
    // the candidate with  #{keys below it} <= tgt < #{keys at or below it}; equal keys are equal bits: any of them.
    // One candidate at a time, read again from LDS: K^2 comparisons against the registers, not K^4 hoisted ones
#pragma unroll 1
    for (int j = 0; j < K * K; ++j) {
      const unsigned kj = key[h0 + (j / K) * HW + j % K];
      if (kj == PF_NONE) continue;
      unsigned lt = 0, le = 0;
#pragma unroll
      for (int q = 0; q < K * K; ++q) {
        lt += ks[q] < kj;
        le += ks[q] <= kj;
      }
      if (lt <= tgt && tgt < le) res = kj;
    }
    *dst = __uint_as_float(spk_unkey(res));
  }
}

inline bool pf_frame_ok(const float* d, const float* mask, int B, int Hc, int Wc, int y0, int rows, int cols, float mask_min) {
  return d && B > 0 && B <= 65535 && dca_window_ok(Hc, Wc, y0, rows, cols) && (long)rows * cols < (1L << 31) &&
         !(mask && mask_min != mask_min);
}

}  // namespace

extern "C" int dca_speckle_filter(const float* d, const float* mask, float* out_disp, float* out_valid, int* out_size,
                                  int* label, int* count, int B, int Hc, int Wc, int y0, int rows, int cols, int max_size,
                                  float max_diff, float mask_min, float fill, hipStream_t stream) {
  DCA_REQUIRE(pf_frame_ok(d, mask, B, Hc, Wc, y0, rows, cols, mask_min));
  DCA_REQUIRE(out_valid && label && count && ((uintptr_t)label & 3) == 0 && ((uintptr_t)count & 3) == 0);
  DCA_REQUIRE(max_size >= 0 && max_diff >= 0.f && max_diff < INFINITY);
  const PfFrame f = {d, mask, Hc, Wc, y0, rows, cols, mask_min};
  const SpkOut o = {out_disp, out_valid, out_size, max_size, fill};
  const int tiles_x = cdiv(cols, PF_TW), tiles_y = cdiv(rows, PF_TH);
  const long tiles = (long)tiles_x * tiles_y;
  const int n = rows * cols;
  const long pairs = (long)(tiles_x - 1) * rows + (long)(tiles_y - 1) * cols;      // < 2 rows cols / 16
  const unsigned per_pixel = (unsigned)cdiv(n, PF_THREADS);
  hipLaunchKernelGGL(spk_local_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(PF_THREADS), 0, stream, f, max_diff, tiles_x,
                     label, count);
  if (pairs > 0) {
    hipLaunchKernelGGL(spk_merge_kernel, dim3((unsigned)cdiv(pairs, PF_THREADS), (unsigned)B), dim3(PF_THREADS), 0, stream, f,
                       max_diff, tiles_x, (int)pairs, label);
    hipLaunchKernelGGL(spk_count_kernel, dim3(per_pixel, (unsigned)B), dim3(PF_THREADS), 0, stream, n, label, count);
  }
  hipLaunchKernelGGL(spk_apply_kernel, dim3(per_pixel, (unsigned)B), dim3(PF_THREADS), 0, stream, f, (const int*)label,
                     (const int*)count, o);
  return dca_launch_status();
}

extern "C" int dca_median_filter(const float* d, const float* mask, float* out, int B, int Hc, int Wc, int y0, int rows,
                                 int cols, int ksize, float mask_min, hipStream_t stream) {
  DCA_REQUIRE(pf_frame_ok(d, mask, B, Hc, Wc, y0, rows, cols, mask_min));
  DCA_REQUIRE(out && out != d && (ksize == 3 || ksize == 5));
  const PfFrame f = {d, mask, Hc, Wc, y0, rows, cols, mask_min};
  const int tiles_x = cdiv(cols, PF_TW);
  const dim3 grid((unsigned)((long)tiles_x * cdiv(rows, PF_TH)), (unsigned)B);
  if (ksize == 3)
    hipLaunchKernelGGL(median_kernel<3>, grid, dim3(PF_THREADS), 0, stream, f, tiles_x, out);
  else
    hipLaunchKernelGGL(median_kernel<5>, grid, dim3(PF_THREADS), 0, stream, f, tiles_x, out);
  return dca_launch_status();
}
