// Stixels: per-column ground / object / sky segments from disparity (nothing in the reference computes
// them): the definition of include/dca_hip.h (dca_stixels) as it is written, the arithmetic itself in stixel_math.h, which the
// host check tools/stixel_math_check.cpp compiles too.
//
// Two launches, the kernel boundary being the only global synchronisation:
//  1. cells:  one thread per cell (consecutive lanes consecutive stixel columns of one cell row): the lower median of the
//             cell's valid quantised disparities by descent over the value's bits -- the cell's width x row_step pixels are
//             counted once per bit, no array is kept -- and the road's disparity at the cell's centre; (q, g) leave as ONE
//             32-bit word of two int16.
//  2. dp:     one WAVE per stixel column, grid (CS, B).  The column's prefix arrays are built in LDS by a wave scan; then kt
//             walks upward: the lanes share the candidates kb, form the segment's cost in O(1) from the prefixes, add it to
//             what sx_open stored for kb when the cells below kb were done (the minimum over the class below, as a key), and
//             the three packed keys are reduced by cross-lane minima -- no barrier between waves, because there is one wave.  The
//             walk back is the kernel's tail: lane 0 follows the back-pointers (LDS) into a segment list (LDS), then all
//             lanes write the dense maps, the list, the count and the energy.
// The plane record another launch wrote is read with device-coherent vector loads.
#include "dca_common.h"
#include "../../include/dca_hip.h"
#include "stixel_math.h"

#pragma clang fp contract(off)

namespace {

#define SX_THREADS 256
static_assert(DCA_STIXEL_MAX_CELLS == 1024, "the key keeps kb in 10 bits");
static_assert(DCA_STIXEL_MAX_CONST == SX_MAX_CONST, "stixel_math.h states the bound for this value");
static_assert(DCA_STIXEL_MAX_WIDTH * DCA_STIXEL_MAX_ROW_STEP <= 128, "a cell has at most 128 pixels");

// B maps (B,Hc,Wc) with the window rows x cols at frame row y0, column 0 of every image (as ground.hip has it)
struct SxFrame {
  const float* d;
  const float* mask;                                         // indexed like d, or NULL
  int Hc, Wc, y0, rows, cols, NB;
  float min_disp, mask_min;
  __device__ __forceinline__ long at(int b, int r, int c) const { return ((long)b * Hc + (y0 + r)) * (long)Wc + c; }
  __device__ __forceinline__ bool valid(long i, int& q) const {
    return gm_valid(d[i], min_disp, NB, &q) && (!mask || mask[i] >= mask_min);
  }
};

struct SxGrid {
  int H, CS, width, row_step, min_valid, max_segments;
};

__device__ __forceinline__ double sx_loadd(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// ---- 1. cells: grid (ceil(H CS / SX_THREADS), B); cells (B,H,CS) words of (q | g << 16) --------------------------------------
__global__ __launch_bounds__(SX_THREADS) void sx_cells_kernel(SxFrame f, SxGrid g, const double* plane, unsigned* __restrict__ cells,
                                                              int nbits) {
  const int b = blockIdx.y, i = blockIdx.x * SX_THREADS + threadIdx.x;
  if (i >= g.H * g.CS) return;
  const int k = i / g.CS, s = i - k * g.CS;
  const double* P = plane + (long)b * DCA_GROUND_PLANE_LEN;
  const float a32 = (float)sx_loadd(P + 0), b32 = (float)sx_loadd(P + 1), c32 = (float)sx_loadd(P + 2);
  const int r0 = sx_cell_row0(k, f.rows, g.row_step), c0 = sx_cell_col0(s, g.width);
  auto count_below = [&](int t) {
    int n = 0;
    for (int dy = 0; dy < g.row_step; ++dy) {
      const long row = f.at(b, r0 + dy, c0);
      for (int dx = 0; dx < g.width; ++dx) {
        int q;
        n += (f.valid(row + dx, q) && q < t) ? 1 : 0;
      }
    }
    return n;
  };
  const int n = count_below(16 * f.NB);                      // every valid q is below 16 NB
  int q = -1;
  if (n >= g.min_valid) q = sx_rank_select(nbits, (n - 1) / 2, count_below);
  const int gq = sx_ground_q(a32, b32, c32, sx_centre_col(s, g.width) - f.cols / 2, sx_centre_row(k, f.rows, g.row_step) - f.rows / 2,
                             f.NB);
  cells[(long)b * g.H * g.CS + i] = ((unsigned)q & 0xffffu) | ((unsigned)gq << 16);
}

struct SxOut {
  unsigned char* seg_class;
  float* seg_disp;
  int* count;
  int* stixels;
  long long* energy;
};

// bytes of LDS for a column of H cells: Hp = H + 1 entries of S2 (int64), the four columns of sx_open (64-bit keys), S1, G, K
// (32 bits; the segment list takes G's place after the last step), N and g (16 bits), then 3 H back-pointers of 16 bits
inline size_t sx_lds_bytes(int H) { return (size_t)(H + 1) * (5 * 8 + 3 * 4 + 2 * 2) + (size_t)H * 3 * 2; }

template <class T>
__device__ __forceinline__ T sx_scan(T v, int lane) {        // inclusive, over the wave
#pragma unroll
  for (int o = 1; o < DCA_WAVE; o <<= 1) {
    const T up = __shfl_up(v, o, DCA_WAVE);
    v += lane >= o ? up : (T)0;
  }
  return v;
}

// ---- 2. the dynamic programme and the walk back: grid (CS, B), one wave -----------------------------------------------------
__global__ __launch_bounds__(DCA_WAVE) void sx_dp_kernel(const unsigned* __restrict__ cells, const double* plane, SxParams P,
                                                         SxGrid g, SxOut o, int rows) {
  extern __shared__ long long sx_lds[];
  __shared__ int sx_count;
  const int lane = threadIdx.x, s = blockIdx.x, b = blockIdx.y, H = g.H, CS = g.CS, Hp = H + 1, MAXS = g.max_segments;
  const long col = (long)b * CS + s;
  const double* R = plane + (long)b * DCA_GROUND_PLANE_LEN;
  const bool ok = sx_loadd(R + 5) != 1.0 && (float)sx_loadd(R + 9) > 0.f;
  if (!ok) {                                                 // the whole launch's image: no segmentation
    if (o.seg_class)
      for (int k = lane; k < H; k += DCA_WAVE) o.seg_class[((long)b * H + k) * CS + s] = DCA_STIXEL_NO_CLASS;
    if (o.seg_disp)
      for (int k = lane; k < H; k += DCA_WAVE) o.seg_disp[((long)b * H + k) * CS + s] = 0.f;
    if (o.stixels)
      for (int j = lane; j < MAXS * 4; j += DCA_WAVE) o.stixels[col * MAXS * 4 + j] = 0;
    if (lane == 0) {
      if (o.count) o.count[col] = 0;
      if (o.energy) o.energy[col] = 0;
    }
    return;
  }
  long long* S2 = sx_lds;
  unsigned long long* O0 = (unsigned long long*)(S2 + Hp);   // O_j[kb] = open[j] of sx_open for a segment that starts at kb
  unsigned long long* O1 = O0 + Hp;
  unsigned long long* O2 = O1 + Hp;
  unsigned long long* O3 = O2 + Hp;
  int* S1 = (int*)(O3 + Hp);
  unsigned* G = (unsigned*)(S1 + Hp);
  unsigned* K = G + Hp;
  unsigned short* N = (unsigned short*)(K + Hp);             // at most 1024 valid cells
  short* gq = (short*)(N + Hp);                              // |g| <= 16384
  unsigned short* back = (unsigned short*)(gq + Hp);         // back[c * H + kt] = kb << 2 | cp
  unsigned* segl = G;                                        // the walk back's list: G is done with by then

  // prefixes over the cells [0, k): entry 0 is zero
  if (lane == 0) {
    const long long none[3] = {0, 0, 0};
    unsigned long long open[4];
    sx_open(P, 0, none, open);
    O0[0] = open[0], O1[0] = open[1], O2[0] = open[2], O3[0] = open[3];
    S2[0] = 0, N[0] = 0, S1[0] = 0, G[0] = 0, K[0] = 0;
  }
  int cn = 0, cs1 = 0;
  long long cs2 = 0;
  unsigned cg = 0, ck = 0;
  for (int base = 0; base < H; base += DCA_WAVE) {
    const int k = base + lane;
    const bool act = k < H;
    const unsigned word = act ? cells[((long)b * H + k) * CS + s] : 0xffffu;
    const int q = (int)(short)(word & 0xffffu), gk = (int)(short)(word >> 16);
    const bool v = q >= 0;
    const int qq = v ? q : 0;
    const int n = sx_scan<int>(v ? 1 : 0, lane) + cn;
    const int s1 = sx_scan<int>(qq, lane) + cs1;
    const long long s2 = sx_scan<long long>((long long)qq * qq, lane) + cs2;
    const unsigned tg = sx_scan<unsigned>(v ? sx_ground_term(q, gk, P.Tg) : 0u, lane) + cg;
    const unsigned ts = sx_scan<unsigned>(v ? sx_sky_term(q, P.Ts) : 0u, lane) + ck;
    if (act) {
      N[k + 1] = (unsigned short)n, S1[k + 1] = s1, S2[k + 1] = s2, G[k + 1] = tg, K[k + 1] = ts;
      gq[k] = (short)gk;
    }
    cn = __shfl(n, DCA_WAVE - 1, DCA_WAVE), cs1 = __shfl(s1, DCA_WAVE - 1, DCA_WAVE), cs2 = __shfl(s2, DCA_WAVE - 1, DCA_WAVE);
    cg = __shfl(tg, DCA_WAVE - 1, DCA_WAVE), ck = __shfl(ts, DCA_WAVE - 1, DCA_WAVE);
  }
  __syncthreads();

  // H dependent steps; key[c] of step kt holds cost[kt][c] and its back-pointer in every lane
  unsigned long long key[3] = {SX_NO_KEY, SX_NO_KEY, SX_NO_KEY};
  for (int kt = 0; kt < H; ++kt) {
    const int nT = N[kt + 1], s1T = S1[kt + 1];
    const long long s2T = S2[kt + 1];
    const unsigned gT = G[kt + 1], kT = K[kt + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) key[c] = SX_NO_KEY;
    for (int base = 0; base <= kt; base += DCA_WAVE) {
      const bool act = base + lane <= kt;
      const int kb = act ? base + lane : 0;                  // a lane beyond kt computes candidate 0 again and drops it
      const unsigned long long open[4] = {O0[kb], O1[kb], O2[kb], O3[kb]};
      unsigned long long cand[3] = {SX_NO_KEY, SX_NO_KEY, SX_NO_KEY};
      sx_relax(P, nT - (int)N[kb], s1T - S1[kb], s2T - S2[kb], (long long)(gT - G[kb]), (long long)(kT - K[kb]), (int)gq[kb], open,
               cand);
#pragma unroll
      for (int c = 0; c < 3; ++c) key[c] = sx_key_min(key[c], act ? cand[c] : SX_NO_KEY);
    }
#pragma unroll
    for (int off = DCA_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) key[c] = sx_key_min(key[c], __shfl_xor(key[c], off, DCA_WAVE));
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) back[c * H + kt] = (unsigned short)(key[c] & 0xfffu);
      if (kt + 1 < H) {                                      // what a segment that starts above this cell finds below it
        const long long prev[3] = {sx_key_cost(key[0]), sx_key_cost(key[1]), sx_key_cost(key[2])};
        unsigned long long open[4];
        sx_open(P, kt + 1, prev, open);
        O0[kt + 1] = open[0], O1[kt + 1] = open[1], O2[kt + 1] = open[2], O3[kt + 1] = open[3];
      }
    }
    __syncthreads();
  }
  const long long top[3] = {sx_key_cost(key[0]), sx_key_cost(key[1]), sx_key_cost(key[2])};

  // the walk back: from the top, at most H segments
  const int ctop = sx_top_class(top[0], top[1], top[2]);
  if (lane == 0) {
    int kt = H - 1, c = ctop, cnt = 0;
    while (cnt < H) {
      const int bp = back[c * H + kt], kb = bp >> 2;
      segl[cnt++] = (unsigned)kb | (unsigned)kt << 10 | (unsigned)c << 20;
      if (kb == 0) break;
      kt = kb - 1, c = bp & 3;
    }
    sx_count = cnt;
    if (o.count) o.count[col] = cnt;
    if (o.energy) o.energy[col] = ctop == 0 ? top[0] : (ctop == 1 ? top[1] : top[2]);
  }
  __syncthreads();
  const int cnt = sx_count;
  for (int i = lane; i < cnt; i += DCA_WAVE) {               // segment i from the top is segment cnt - 1 - i from the bottom
    const unsigned e = segl[i];
    const int kb = (int)(e & 1023u), kt = (int)(e >> 10 & 1023u), c = (int)(e >> 20), j = cnt - 1 - i;
    const int mu = c == SX_OBJECT ? sx_mu(N[kt + 1] - N[kb], S1[kt + 1] - S1[kb]) : -1;
    const float disp = mu >= 0 ? (float)mu / 16.0f : 0.f;
    for (int k = kb; k <= kt; ++k) {
      if (o.seg_class) o.seg_class[((long)b * H + k) * CS + s] = (unsigned char)c;
      if (o.seg_disp) o.seg_disp[((long)b * H + k) * CS + s] = disp;
    }
    if (o.stixels && j < MAXS) {
      int* st = o.stixels + (col * MAXS + j) * 4;
      st[0] = sx_cell_row0(kt, rows, g.row_step), st[1] = sx_cell_row0(kb, rows, g.row_step) + g.row_step - 1, st[2] = c, st[3] = mu;
    }
  }
  if (o.stixels)
    for (int j = cnt * 4 + lane; j < MAXS * 4; j += DCA_WAVE) o.stixels[col * MAXS * 4 + j] = 0;
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }
inline bool sx_const_ok(int v) { return v >= 0 && v <= DCA_STIXEL_MAX_CONST; }

}  // namespace

extern "C" int dca_stixels(const float* d, const float* mask, const double* plane, short* ws, short* cells,
                           unsigned char* seg_class, float* seg_disp, int* count, int* stixels, long long* energy, int B, int Hc,
                           int Wc, int y0, int rows, int cols, int max_disp, int width, int row_step, int min_valid,
                           int max_segments, float min_disp, float mask_min, int Tg, int Ts, int eps, int below, int hang,
                           int mu_min, int far, int seg0, int seg1, int seg2, int first0, int first1, int first2, int t00,
                           int t01, int t02, int t10, int t11, int t12, int t20, int t21, int t22, hipStream_t stream) {
  DCA_REQUIRE(d && plane && ((uintptr_t)plane & 7) == 0 && B > 0 && B <= 65535 && dca_window_ok(Hc, Wc, y0, rows, cols));
  DCA_REQUIRE(rows <= DCA_GROUND_MAX_DIM && cols <= DCA_GROUND_MAX_DIM && max_disp >= 8 && max_disp <= DCA_GROUND_MAX_DISP);
  DCA_REQUIRE(min_disp >= 0.f && finite_f(min_disp) && !(mask && mask_min != mask_min));
  DCA_REQUIRE(width >= 1 && width <= DCA_STIXEL_MAX_WIDTH && row_step >= 1 && row_step <= DCA_STIXEL_MAX_ROW_STEP);
  const int H = rows / row_step, CS = cols / width;
  DCA_REQUIRE(H >= 2 && H <= DCA_STIXEL_MAX_CELLS && CS >= 1 && min_valid >= 1 && min_valid <= width * row_step);
  DCA_REQUIRE(max_segments >= 1 && max_segments <= DCA_STIXEL_MAX_SEGMENTS);
  const bool segment = seg_class || seg_disp || count || stixels || energy;
  DCA_REQUIRE(segment || cells);
  unsigned* cell_words = (unsigned*)(cells ? cells : ws);
  DCA_REQUIRE(cell_words && ((uintptr_t)cell_words & 3) == 0);
  DCA_REQUIRE(((uintptr_t)seg_disp & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)stixels & 3) == 0 &&
              ((uintptr_t)energy & 7) == 0);
  const SxParams P = {Tg, Ts, eps, below, hang, mu_min, far, {seg0, seg1, seg2}, {first0, first1, first2},
                      {{t00, t01, t02}, {t10, t11, t12}, {t20, t21, t22}}};
  DCA_REQUIRE(sx_const_ok(Tg) && sx_const_ok(Ts) && sx_const_ok(eps) && sx_const_ok(below) && sx_const_ok(hang) &&
              sx_const_ok(mu_min) && sx_const_ok(far));
  for (int c = 0; c < 3; ++c) {
    DCA_REQUIRE(sx_const_ok(P.seg[c]) && sx_const_ok(P.first[c]));
    for (int cp = 0; cp < 3; ++cp) DCA_REQUIRE(P.T[cp][c] >= -1 && P.T[cp][c] <= DCA_STIXEL_MAX_CONST);
  }
  const SxFrame fr = {d, mask, Hc, Wc, y0, rows, cols, max_disp, min_disp, mask_min};
  const SxGrid g = {H, CS, width, row_step, min_valid, max_segments};
  hipLaunchKernelGGL(sx_cells_kernel, dim3((unsigned)cdiv((long)H * CS, SX_THREADS), (unsigned)B), dim3(SX_THREADS), 0, stream, fr,
                     g, plane, cell_words, sx_value_bits(max_disp));
  if (segment) {
    const SxOut o = {seg_class, seg_disp, count, stixels, energy};
    hipLaunchKernelGGL(sx_dp_kernel, dim3((unsigned)CS, (unsigned)B), dim3(DCA_WAVE), sx_lds_bytes(H), stream,
                       (const unsigned*)cell_words, plane, P, g, o, rows);
  }
  return dca_launch_status();
}
