// The persistent tile walk of the 3x3x3 convolution family: the ONLY statement of which workgroup visits which tile,
// of how a tile index becomes coordinates, and of how many tiles a problem has.  Shared by conv3d_f16x2, conv3d_bf16x3,
// conv3d_lp, conv3d_s2_f16x2, conv3d_s2_lp, deconv3d_x3, deconv3d_lp and the three split weight gradients; the host can
// call the walk too (dca_tile_walk, abi.hip), which is how tests/test_wgrad_cases_cpu.py checks the partition property
// on the arithmetic the kernels run.
#pragma once
#include <hip/hip_runtime.h>

// tiles begin, begin + step, ... < end of one workgroup
struct DcaTileWalk {
  int begin, end, step;
};

// persistent: the tile space (w fastest) is cut into one contiguous range per XCD (workgroups are dealt round-robin
// over the 8 XCDs, each with its own L2); inside its XCD's range, workgroup j of cnt takes tiles j, j + cnt, ... so
// at any time the CUs of an XCD work on neighbouring tiles and share their halos in that L2.  The load / MFMA
// pipeline runs straight across tile boundaries.
// grid and wg are unsigned like gridDim.x / blockIdx.x: signed parameters turn the divisions below into signed ones
// and change thousands of lines of every kernel's code.
__host__ __device__ __forceinline__ DcaTileWalk dca_tile_walk_of(long T, unsigned grid, unsigned wg) {
  const int nx = grid >= 8 ? 8 : 1, xcd = wg % nx;
  const int cnt = (grid - xcd + nx - 1) / nx;          // workgroups on this XCD
  DcaTileWalk w;
  w.begin = (int)(T * xcd / nx) + wg / nx; w.end = (int)(T * (xcd + 1) / nx); w.step = cnt;
  return w;
}
// the walk of this workgroup (grid x = the persistent workgroups)
__device__ __forceinline__ DcaTileWalk dca_my_tile_walk(long T) { return dca_tile_walk_of(T, gridDim.x, blockIdx.x); }

// tile index -> sample n and the tile's first output voxel (d0, h0, w0); tiles of TD x TH x TW voxels, w fastest
template <int TD, int TH, int TW>
__host__ __device__ __forceinline__ void dca_tile_decode(int tile, int nTD, int nTH, int nTW, int& n, int& d0, int& h0, int& w0) {
  const int tw = tile % nTW; tile /= nTW;
  const int th = tile % nTH; tile /= nTH;
  const int td = tile % nTD;
  n = tile / nTD;
  d0 = td * TD; h0 = th * TH; w0 = tw * TW;
}

// A step of a software pipeline that runs across tile boundaries: channel chunk `chunk` of tile `tile` (deconv3d_x3
// counts its (chunk, kd) steps there, 3 NCH per tile).  tile >= walk.end marks "none".
struct DcaTileStep {
  int tile, chunk, n, d0, h0, w0;
};
template <int TD, int TH, int TW>
__host__ __device__ __forceinline__ void dca_tile_advance(DcaTileStep& c, int nchunk, const DcaTileWalk& walk, int nTD, int nTH,
                                                          int nTW) {
  if (c.chunk + 1 < nchunk) { ++c.chunk; return; }
  c.chunk = 0;
  c.tile += walk.step;
  if (c.tile < walk.end) dca_tile_decode<TD, TH, TW>(c.tile, nTD, nTH, nTW, c.n, c.d0, c.h0, c.w0);
}

// ---- host: the tile grid of a problem ----------------------------------------------------------------------------------
// Tile indices are ints in the kernels: a launcher requires fits() before it launches (a size query has no error to
// return and reports what the arithmetic gives).
constexpr long DCA_TILES_END = 0x7fffffffL;
struct DcaTileGrid {
  int nTD, nTH, nTW;
  long tiles;
  bool fits() const { return tiles < DCA_TILES_END; }
};
template <int TD, int TH, int TW>
static inline DcaTileGrid dca_tile_grid(int N, int D, int H, int W) {
  DcaTileGrid t;
  t.nTD = (D + TD - 1) / TD; t.nTH = (H + TH - 1) / TH; t.nTW = (W + TW - 1) / TW;
  t.tiles = (long)N * t.nTD * t.nTH * t.nTW;
  return t;
}
