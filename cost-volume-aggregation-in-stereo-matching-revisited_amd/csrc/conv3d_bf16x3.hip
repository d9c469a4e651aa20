// 3x3x3 stride-1 convolution on the bf16 matrix pipe with fp32-grade accuracy ("bf16x3" split emulation).
//
// Every fp32 operand is split exactly into three bf16 terms, x = h + m + l (h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m); the residuals are exact in fp32, so the three terms carry 24 significand bits), and a product
// w*x is evaluated as the six partial products whose weight is >= 2^-16:
//     w_h x_h + (w_h x_m + w_m x_h) + (w_h x_l + w_m x_m + w_l x_h)
// Each partial product is exact in the MFMA's fp32 accumulator; the dropped terms (w_m x_l, w_l x_m, w_l x_l) are
// <= 2^-23 relative, the size of one fp32 rounding.  No range restriction: bf16 has the fp32 exponent.
// Six v_mfma_f32_32x32x16_bf16 (32 cycles each, K = 16) replace sixteen v_mfma_f32_32x32x2f32 (64 cycles each) per
// 32 input channels, tap and 32-voxel tile: 2.67x fewer matrix-pipe cycles than the fp32 kernel of conv3d_mfma.hip,
// which is pinned to its matrix-pipe ceiling.
//
// Reference operators served: nn.Conv3d(k=3, s=1, p=1) of convbn_3d (models/submodule.py:121-124) in dres0/dres1,
// Multi_Aggregation and the cva blocks (models/augment/cva.py:13-55), and their backward-data.
//
// Work decomposition: one workgroup (8 waves) per 4 x 8 x 16 output tile (512 voxels = 16 MFMA column tiles, two per
// wave) and 32 output channels; one workgroup per CU (LDS bound), two waves per SIMD.  Input channels go through LDS
// in chunks of 16 (one MFMA K): the 6 x 10 x 18 halo tile of the chunk, pre-split into three bf16 images laid out
// [term][k half][voxel][8 bf16] so that a lane's B fragment (8 consecutive k of its voxel) is one ds_read_b128 and 16
// consecutive lanes read 256 contiguous bytes.  The weights arrive pre-split and pre-swizzled into MFMA A fragments
// (x3_prep_weight_kernel) and stream through a double-buffered LDS slab of 9 taps (one kd plane) per phase, so a
// channel chunk is three phases of 108 MFMAs per wave with one barrier each; the next slab / next halo tile are
// fetched into registers (hardware-predicated buffer loads) while the current phase's MFMAs run.
#include "dca_frag.h"
#include "dca_tiles.h"
#include "bn_fused_stats.h"
#include <type_traits>

// The output stores of this family (this kernel, conv3d_f16x2.hip, conv3d_lp.hip, deconv3d_x3.hip) are PLAIN stores.
// Non-temporal ones were measured here: y is written once, so it need not displace the halo lines the neighbouring tiles
// re-read from this XCD's L2 -- 591 -> 568 us on the fused-epilogue 32->32 launch at 48x136x240 in isolation.  In the
// network the consumer of y (BatchNorm statistics + apply in training, the next convolution in inference) runs right
// behind and finds a 200 MB output partly in the 256 MB infinity cache when it was stored with the default policy: with
// non-temporal stores the training step went 37.38 -> 37.86 ms per pair at batch 1, the eval forward 7.51 -> 7.63 ms, the
// batch-4 step 143.4 -> 143.7 ms.  (The switchable builds and their scripts are in history before this commit.)

namespace {

constexpr int TD = 4, TH = 8, TW = 16;
constexpr int ID = TD + 2, IH = TH + 2, IW = TW + 2;
constexpr int NVOX = ID * IH * IW;                 // 1080 halo voxels
constexpr int B_TERM = 2 * NVOX * 16;              // bytes of one bf16 term image (2 k halves x voxels x 16 B)
constexpr int B_BYTES = 3 * B_TERM;                // 103680
constexpr int A_SLAB = 9 * 3 * 1024;               // 9 taps x 3 terms x (64 lanes x 16 B)
constexpr int LDS_BYTES = B_BYTES + 2 * A_SLAB;    // 158976 of the CU's 163840
constexpr int NB_ITEMS = 2 * NVOX;                 // (k half, voxel) staging items of 8 channels (unaligned path)
constexpr int KB = (NB_ITEMS + 511) / 512;         // 5
constexpr int NROWS = 2 * ID * IH;                 // 120 (k half, d, h) halo rows: 4 aligned quads + 2 edge voxels each
constexpr int NQUAD = NROWS * 4, NEDGE = NROWS * 2;  // aligned path: 480 quad items (8 x b128), 240 edge items (8 x b32)
static_assert(NQUAD <= 512 && NEDGE <= 512, "one quad / edge item per thread");
constexpr int NA_ITEMS = A_SLAB / 16;              // 1728 b128 per slab
constexpr int KA = (NA_ITEMS + 511) / 512;         // 4

struct X3Args {
  const float* x;
  const unsigned short* wx;
  float* y;
  const float* scale;
  const float* shift;
  const float* res_pre;
  const float* res_post;
  float slope;
  int N, Cin, Cout, NCH;
  int D, H, W;
  int nTD, nTH, nTW;
  double* stat_part;         // STATS: one partial {K, n, s, q} per (channel, workgroup): bn_fused_stats.h
};

constexpr int STAT_LDS = 8 * FS_WAVE_FLOATS * 4;

// STATS: the raw convolution output feeds a training-mode BatchNorm -- the kernel also produces, per channel and workgroup,
// the partial statistics {K, n, sum (y - K), sum (y - K)^2} that dca_bn_finalize_centered consumes (bn_fused_stats.h), so the
// 200 MB statistics pass over y disappears.  Per tile: 3 vector instructions per output value, a DPP reduction over the 32
// positions of a wave half, one ds_add_f32 per (half, channel) into a wave-private LDS slot.
template <bool VEC, bool STATS>
__global__ __launch_bounds__(512) void conv3_bf16x3_kernel(X3Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* b_lds = smem;
  char* a_lds = smem + B_BYTES;
  float* stat_lds = (float*)(smem + LDS_BYTES);     // STATS only (the launch adds STAT_LDS bytes)

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int cblk = blockIdx.y;
  // persistent: the tile space (w fastest) is cut into one contiguous range per XCD (workgroups are dealt round-robin
  // over the 8 XCDs, each with its own L2); inside its XCD's range, workgroup j of cnt takes tiles j, j + cnt, ... so
  // at any time the CUs of an XCD work on neighbouring tiles and share their halos in that L2.  The load / MFMA
  // pipeline runs straight across tile boundaries.
  const DcaTileWalk walk = dca_my_tile_walk((long)a.N * a.nTD * a.nTH * a.nTW);   // dca_tiles.h
  const int t_begin = walk.begin, t_end = walk.end, t_step = walk.step;
  float* stat_w = stat_lds + wv * FS_WAVE_FLOATS;   // this wave's slots
  bool stat_first = true;
  if constexpr (STATS) {
    for (int i = tid; i < 8 * FS_WAVE_FLOATS; i += 512) stat_lds[i] = 0.f;
    __syncthreads();
  }
  if (t_begin >= t_end) {
    if constexpr (STATS) fs_flush(stat_lds, 8, tid, cblk * 32, a.Cout, a.stat_part, gridDim.x, blockIdx.x);
    return;
  }

  // per-lane byte offset of the lane's voxel inside a term image, for its two column tiles
  // ds_read_b128 is served in four NON-contiguous 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...:
  // MI355X_MICROARCH.md, LDS).  A column tile is two h-rows of 16 voxels; the second row starts IW*16 = 288 B = 32 B
  // (mod 256) after the first, which put lanes 20-27 on the banks of lanes 12-15 (2-way conflict in every group: 39 % of
  // this kernel's LDS cycles were SQ_LDS_BANK_CONFLICT).  Rotating the second row's w by -2 voxels makes the bank pattern of
  // lanes 16-31 equal to that of a contiguous 1 KiB read: conflict free.  The epilogue uses the same lane -> w map.
  const int wlane = (l31 & 16) ? (((l31 & 15) - 2) & 15) : (l31 & 15);
  int boff[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = (wv * 2 + t) * 2 + (l31 >> 4), dl = r >> 3, hl = r & 7;
    boff[t] = (half * NVOX + (dl * IH + hl) * IW + wlane) * 16;
  }

  const int cstride = a.D * a.H * a.W;
  const long sample = (long)a.Cin * cstride;
  const int P = a.NCH * 3;
  const long wbytes = (long)P * A_SLAB;
  const __amdgpu_buffer_rsrc_t wr = dca_rsrc((const char*)a.wx + (long)cblk * wbytes, wbytes);

  const bool has_aff = a.scale != nullptr, has_pre = a.res_pre != nullptr, has_post = a.res_post != nullptr;
  float4 ra[KA];
  auto load_A = [&](int p) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int it = tid + 512 * k;
      ra[k] = dca_bload4(wr, p * A_SLAB + it * 16, (int)(it < NA_ITEMS));
    }
  };
  auto store_A = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int it = tid + 512 * k;
      if (it < NA_ITEMS) *(float4*)(a_lds + buf * A_SLAB + it * 16) = ra[k];
    }
  };

  // Staging of a chunk's halo tile, global -> registers (load_B) -> split -> LDS (store_B).
  //  VEC (W % 4 == 0, 16-byte aligned x): a thread owns one aligned quad of 4 voxels along W (8 x b128, one per
  //  channel of its k half) and, for tid < 240, one of the two edge voxels of a row (8 x b32): 16 loads per thread.
  //  Otherwise: 5 single-voxel items of 8 x b32.
  float4 rq[VEC ? 8 : 1];
  float re[VEC ? 8 : 1];
  float rb[VEC ? 1 : KB][8];
  int item_crd[VEC ? 2 : KB];  // packed halo coordinates of the thread's items, fixed for the whole kernel
  if constexpr (VEC) {
    {
      const int row = tid >> 2, q = tid & 3, kh = row / (ID * IH), rem = row - kh * (ID * IH), id = rem / IH, ih = rem - id * IH;
      item_crd[0] = (tid < NQUAD) ? (id | (ih << 8) | ((1 + 4 * q) << 16) | (kh << 24)) : -1;
    }
    {
      const int row = tid >> 1, side = tid & 1, kh = row / (ID * IH), rem = row - kh * (ID * IH), id = rem / IH, ih = rem - id * IH;
      item_crd[1] = (tid < NEDGE) ? (id | (ih << 8) | ((side ? IW - 1 : 0) << 16) | (kh << 24)) : -1;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int it = tid + 512 * k;
      const int kh = it / NVOX, v = it - kh * NVOX;
      const int id = v / (IH * IW), rem = v - id * (IH * IW), ih = rem / IW, iw = rem - ih * IW;
      item_crd[k] = (it < NB_ITEMS) ? (id | (ih << 8) | (iw << 16) | (kh << 24)) : -1;
    }
  }
  auto item_off = [&](int crd, int d0, int h0, int w0, int chunk, int& c0, int& okv) __attribute__((always_inline)) {
    const int di = d0 - 1 + (crd & 255), hi = h0 - 1 + ((crd >> 8) & 255), wi = w0 - 1 + ((crd >> 16) & 255);
    c0 = chunk * 16 + ((crd >> 24) & 1) * 8;
    okv = (int)(crd >= 0) & (int)((unsigned)di < (unsigned)a.D) & (int)((unsigned)hi < (unsigned)a.H) &
          (int)((unsigned)wi < (unsigned)a.W);
    return (c0 * cstride + (di * a.H + hi) * a.W + wi) * 4;
  };
  auto load_B = [&](int n, int d0, int h0, int w0, int chunk) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t xr = dca_rsrc(a.x + (long)n * sample, sample * 4);
    if constexpr (VEC) {
      int c0, okv;
      const int offq = item_off(item_crd[0], d0, h0, w0, chunk, c0, okv);  // a quad is inside W or outside as a whole
#pragma unroll
      for (int j = 0; j < 8; ++j) rq[j] = dca_bload4(xr, offq + j * cstride * 4, okv & (int)(c0 + j < a.Cin));
      const int offe = item_off(item_crd[1], d0, h0, w0, chunk, c0, okv);
#pragma unroll
      for (int j = 0; j < 8; ++j) re[j] = dca_bload1(xr, offe + j * cstride * 4, okv & (int)(c0 + j < a.Cin));
    } else {
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        int c0, okv;
        const int off = item_off(item_crd[k], d0, h0, w0, chunk, c0, okv);
#pragma unroll
        for (int j = 0; j < 8; ++j) rb[k][j] = dca_bload1(xr, off + j * cstride * 4, okv & (int)(c0 + j < a.Cin));
      }
    }
  };
  auto split_store = [&](const float (&v)[8], int vox_off) __attribute__((always_inline)) {
    bf16x8 hv, mv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __bf16 h, m, l;
      x3_split(v[j], h, m, l);
      hv[j] = h; mv[j] = m; lv[j] = l;
    }
    *(bf16x8*)(b_lds + vox_off) = hv;
    *(bf16x8*)(b_lds + B_TERM + vox_off) = mv;
    *(bf16x8*)(b_lds + 2 * B_TERM + vox_off) = lv;
  };
  auto crd_lds = [&](int crd) __attribute__((always_inline)) {  // byte offset of the item's (first) voxel in a term image
    return ((((crd >> 24) & 1) * ID + (crd & 255)) * IH + ((crd >> 8) & 255)) * IW * 16 + ((crd >> 16) & 255) * 16;
  };
  auto store_B = [&]() __attribute__((always_inline)) {
    if constexpr (VEC) {
      if (item_crd[0] >= 0) {
        const int o = crd_lds(item_crd[0]);
        const float v0[8] = {rq[0].x, rq[1].x, rq[2].x, rq[3].x, rq[4].x, rq[5].x, rq[6].x, rq[7].x};
        const float v1[8] = {rq[0].y, rq[1].y, rq[2].y, rq[3].y, rq[4].y, rq[5].y, rq[6].y, rq[7].y};
        const float v2[8] = {rq[0].z, rq[1].z, rq[2].z, rq[3].z, rq[4].z, rq[5].z, rq[6].z, rq[7].z};
        const float v3[8] = {rq[0].w, rq[1].w, rq[2].w, rq[3].w, rq[4].w, rq[5].w, rq[6].w, rq[7].w};
        split_store(v0, o); split_store(v1, o + 16); split_store(v2, o + 32); split_store(v3, o + 48);
      }
      if (item_crd[1] >= 0) {
        const float v[8] = {re[0], re[1], re[2], re[3], re[4], re[5], re[6], re[7]};
        split_store(v, crd_lds(item_crd[1]));
      }
    } else {
#pragma unroll
      for (int k = 0; k < KB; ++k)
        if (item_crd[k] >= 0) split_store(rb[k], crd_lds(item_crd[k]));
    }
  };
  auto decode = [&](int tile, int& n, int& d0, int& h0, int& w0) __attribute__((always_inline)) {
    dca_tile_decode<TD, TH, TW>(tile, a.nTD, a.nTH, a.nTW, n, d0, h0, w0);
  };

  int n, d0, h0, w0;
  decode(t_begin, n, d0, h0, w0);
  load_B(n, d0, h0, w0, 0);
  load_A(0);
  store_B();
  store_A(0);
  load_A(1);   // P >= 3
  __syncthreads();

  int buf = 0;  // A slab buffer of the current phase (phases alternate buffers across chunk and tile boundaries)
#pragma unroll 1
  for (int tile = t_begin; tile < t_end; tile += t_step) {
    const bool more_tiles = tile + t_step < t_end;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    int nn = n, nd0 = d0, nh0 = h0, nw0 = w0;  // coordinates of the next tile (valid when more_tiles)

#pragma unroll 1
    for (int p = 0; p < P; ++p, buf ^= 1) {
      const int chunk = p / 3, kd = p - chunk * 3;
      const bool last_of_chunk = kd == 2;
      const bool next_chunk = last_of_chunk && (chunk + 1 < a.NCH);
      const bool next_tile = last_of_chunk && !next_chunk && more_tiles;
      // slab p+1 (in registers since the previous phase) -> the buffer phase p-1 used; then fetch slab p+2
      if (p + 1 < P || more_tiles) store_A(buf ^ 1);
      if (p + 2 < P || more_tiles) load_A(p + 2 < P ? p + 2 : p + 2 - P);
      if (next_tile) decode(tile + t_step, nn, nd0, nh0, nw0);
      const bool stage = next_chunk || next_tile;  // fetch the halo tile of the next chunk / chunk 0 of the next tile
      const char* ab = a_lds + buf * A_SLAB + lane * 16;
      const char* bb = b_lds + kd * (IH * IW * 16);
      // The 9 taps of the slab with a register double buffer: the 9 ds_read_b128 of tap+1 go one per MFMA between
      // the 12 MFMAs of tap, and in a staging phase the global loads of the next halo tile are spread over the taps
      // as well (all issued up front they fill the CU's memory queue and the waves sit in the issue stage for
      // microseconds with the matrix pipe idle).  sched_group_barrier pins the order; left alone, hipcc issues each
      // LDS read right before its first use and waits on it.
      auto phase = [&](auto STAGE) __attribute__((always_inline)) {
        constexpr bool ST = decltype(STAGE)::value;
        constexpr int NLD = VEC ? 2 : 5;  // global loads per tap (8 taps): 16 / 40 per thread
        if constexpr (ST) {
          const bool nt = next_tile;
          load_B(nt ? nn : n, nt ? nd0 : d0, nt ? nh0 : h0, nt ? nw0 : w0, nt ? 0 : chunk + 1);
        }
        bf16x8 fa[2][3], fb[2][2][3];
        auto load_frag = [&](int tap9, int slot) __attribute__((always_inline)) {
          const int kh = tap9 / 3, kw = tap9 - kh * 3;
#pragma unroll
          for (int term = 0; term < 3; ++term) fa[slot][term] = *(const bf16x8*)(ab + (tap9 * 3 + term) * 1024);
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int term = 0; term < 3; ++term)
              fb[slot][t][term] = *(const bf16x8*)(bb + boff[t] + (kh * IW + kw) * 16 + term * B_TERM);
        };
        load_frag(0, 0);
#pragma unroll
        for (int tap9 = 0; tap9 < 9; ++tap9) {
          const int cur = tap9 & 1;
          if (tap9 < 8) load_frag(tap9 + 1, cur ^ 1);
          // smallest terms first; the two column tiles alternate so consecutive MFMAs never chain on one accumulator
          constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
          for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][PA[q]], fb[cur][t][PB[q]], acc[t], 0, 0, 0);
          if (tap9 < 8) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
              if (ST && i < NLD) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
          }
        }
      };
      if (stage) phase(std::true_type{}); else phase(std::false_type{});
      if (stage) {
        __syncthreads();  // every wave is done reading the halo tile of this chunk
        store_B();
      }
      __syncthreads();
    }

    // Epilogue (same contract as conv3d_mfma.hip): y = act(acc * scale + shift + res_pre) + res_post.  The stores
    // drain while the next tile's first phase runs.
    // 32-bit offsets into this sample's output through buffer descriptors: nothing 64-bit for the compiler to hoist
    // out of the tile loop (that cost ~60 spilled registers), and the bounds masks ride on the hardware range check.
    const long osample = (long)a.Cout * cstride;
    const __amdgpu_buffer_rsrc_t yr = dca_rsrc(a.y + (long)n * osample, osample * 4);
    const __amdgpu_buffer_rsrc_t pr = dca_rsrc((has_pre ? a.res_pre : a.y) + (long)n * osample, osample * 4);
    const __amdgpu_buffer_rsrc_t qr = dca_rsrc((has_post ? a.res_post : a.y) + (long)n * osample, osample * 4);
    float sc[16], sh[16];  // (re)loaded per tile: holding them across the MFMA phases costs 32 registers
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = min(cblk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, a.Cout - 1);
      sc[r] = has_aff ? a.scale[co] : 1.f;
      sh[r] = has_aff ? a.shift[co] : 0.f;
    }
    float st_s[STATS ? 16 : 1], st_q[STATS ? 16 : 1], st_n = 0.f;
    if constexpr (STATS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st_s[r] = st_q[r] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r0 = (wv * 2 + t) * 2 + (l31 >> 4), d = d0 + (r0 >> 3), h = h0 + (r0 & 7), w = w0 + wlane;
      const int ok = (int)(d < a.D) & (int)(h < a.H) & (int)(w < a.W);
      if constexpr (STATS) st_n += (float)ok;
      const int voff = ((d * a.H + h) * a.W + w + (cblk * 32 + 4 * half) * cstride) * 4;
      float rp[16], rq[16];
      if (has_pre) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cu = (r & 3) + 8 * (r >> 2);
          rp[r] = dca_bload1(pr, voff + cu * cstride * 4, ok & (int)(cblk * 32 + cu + 4 * half < a.Cout));
        }
      }
      if (has_post) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cu = (r & 3) + 8 * (r >> 2);
          rq[r] = dca_bload1(qr, voff + cu * cstride * 4, ok & (int)(cblk * 32 + cu + 4 * half < a.Cout));
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = (r & 3) + 8 * (r >> 2);
        float v = acc[t][r] * sc[r] + sh[r];
        if (has_pre) v += rp[r];
        v = act_apply(v, a.slope);
        if (has_post) v += rq[r];
        if constexpr (STATS) {
          if (stat_first && t == 0) {   // the wave's first tile: the shift of (half, r) = what lane 0 of the half produced
            const float kf = fs_half_first(v, half);
            if ((lane & 31) == 0) fs_slot(stat_w, half, r)[0] = kf;
          }
          const float dlt = ok ? v - fs_slot(stat_w, half, r)[0] : 0.f;
          st_s[r] += dlt;
          st_q[r] = fmaf(dlt, dlt, st_q[r]);
        }
        dca_bstore1(yr, v, voff + cu * cstride * 4, ok & (int)(cblk * 32 + cu + 4 * half < a.Cout));
      }
    }
    if constexpr (STATS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float rs = fs_half_sum(st_s[r]), rq2 = fs_half_sum(st_q[r]);
        if ((lane & 31) == 0) {
          atomicAdd(fs_slot(stat_w, half, r) + 1, rs);    // ds_add_f32 without return; wave-private slot, one writer lane
          atomicAdd(fs_slot(stat_w, half, r) + 2, rq2);
        }
      }
      const float rn = fs_half_sum(st_n);
      if ((lane & 31) == 0) atomicAdd(stat_w + 96 + half, rn);
      stat_first = false;
    }
    n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
  }
  if constexpr (STATS) {
    __syncthreads();
    fs_flush(stat_lds, 8, tid, cblk * 32, a.Cout, a.stat_part, gridDim.x, blockIdx.x);
  }
}

// the bf16x3 weight fragments wx[cblk][chunk][tap][term][lane][j] (wx3_elem, dca_frag.h)
__global__ void x3_prep_weight_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int A, int Bn,
                                      int NCH, int src_ab, int flip, long total) {
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x)
    dst[idx] = wx3_elem(src, idx, A, Bn, NCH, src_ab, flip);
}

}  // namespace

extern "C" long dca_conv3d_x3_weight_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return (long)((Cout + 31) / 32) * ((Cin + 15) / 16) * 27 * 3 * 1024;
}

extern "C" int dca_conv3d_x3_prep_weight(const float* w, void* wx, int A, int B, int src_ab, int flip,
                                         hipStream_t stream) {
  DCA_REQUIRE(w && wx && A > 0 && B > 0);
  const int NCH = (A + 15) / 16;
  const long total = dca_conv3d_x3_weight_bytes(A, B) / 2;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(x3_prep_weight_kernel, dim3(grid), dim3(256), 0, stream, w, (unsigned short*)wx, A, B, NCH, src_ab,
                     flip, total);
  return dca_launch_status();
}

namespace {

// launch geometry: persistent, one workgroup per CU (the LDS footprint allows no more; gx per block of 32 output channels),
// each looping over its share of the tiles; gx is also the number of statistics partials per channel
struct X3Geom {
  DcaTileGrid t;
  int cblks, gx;
};
X3Geom x3_geometry(int N, int Cout, int D, int H, int W) {
  X3Geom g;
  g.t = dca_tile_grid<TD, TH, TW>(N, D, H, W);
  g.cblks = (Cout + 31) / 32;
  g.gx = dca_persistent_grid(g.t.tiles, g.cblks);
  return g;
}

int x3_launch(const float* x, const void* wx, float* y, const float* scale, const float* shift, const float* res_pre,
              const float* res_post, float slope, double* stat_part, int N, int Cin, int Cout, int D, int H, int W,
              hipStream_t stream) {
  DCA_REQUIRE(x && wx && y && N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0);
  DCA_REQUIRE((scale == nullptr) == (shift == nullptr));
  DCA_REQUIRE((long)Cin * D * H * W * 4 < 0x7ffffff0L && (long)Cout * D * H * W * 4 < 0x7ffffff0L);  // 32-bit byte offsets inside one sample
  DCA_REQUIRE((((uintptr_t)wx) & 15) == 0);
  X3Args a;
  a.x = x; a.wx = (const unsigned short*)wx; a.y = y;
  a.scale = scale; a.shift = shift; a.res_pre = res_pre; a.res_post = res_post; a.slope = slope;
  a.N = N; a.Cin = Cin; a.Cout = Cout; a.NCH = (Cin + 15) / 16;
  a.D = D; a.H = H; a.W = W;
  const X3Geom g = x3_geometry(N, Cout, D, H, W);
  a.nTD = g.t.nTD; a.nTH = g.t.nTH; a.nTW = g.t.nTW;
  a.stat_part = stat_part;
  DCA_REQUIRE(g.t.fits() && g.cblks <= 65535);
  const bool vec = (W % 4 == 0) && ((((uintptr_t)x) & 15) == 0);
  const bool stats = stat_part != nullptr;
  auto kern = stats ? (vec ? conv3_bf16x3_kernel<true, true> : conv3_bf16x3_kernel<false, true>)
                    : (vec ? conv3_bf16x3_kernel<true, false> : conv3_bf16x3_kernel<false, false>);
  const int lds = LDS_BYTES + (stats ? STAT_LDS : 0);
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kern, dim3(g.gx, g.cblks), dim3(512), lds, stream, a);
  return dca_launch_status();
}

}  // namespace

extern "C" int dca_conv3d_x3_forward(const float* x, const void* wx, float* y, const float* scale, const float* shift,
                                     const float* res_pre, const float* res_post, float slope, int N, int Cin, int Cout,
                                     int D, int H, int W, hipStream_t stream) {
  return x3_launch(x, wx, y, scale, shift, res_pre, res_post, slope, nullptr, N, Cin, Cout, D, H, W, stream);
}

// nchunk of the statistics dca_conv3d_x3_forward_stats produces (one partial per workgroup of the launch it will make)
extern "C" long dca_conv3d_x3_stats_chunks(int N, int Cout, int D, int H, int W) {
  if (N <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return x3_geometry(N, Cout, D, H, W).gx;
}

// y = conv(x, w) (no epilogue) plus the BatchNorm batch statistics of y: part (Cout * nchunk * 4 doubles, nchunk =
// dca_conv3d_x3_stats_chunks) = one {K, n, sum (y - K), sum (y - K)^2} per (channel, workgroup), for
// dca_bn_finalize_centered (bn_fused_stats.h)
extern "C" int dca_conv3d_x3_forward_stats(const float* x, const void* wx, float* y, double* stat_part, int N, int Cin,
                                           int Cout, int D, int H, int W, hipStream_t stream) {
  DCA_REQUIRE(stat_part);
  return x3_launch(x, wx, y, nullptr, nullptr, nullptr, nullptr, 1.f, stat_part, N, Cin, Cout, D, H, W, stream);
}
