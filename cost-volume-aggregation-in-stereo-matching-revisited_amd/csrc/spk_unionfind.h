// Union-find of the speckle filter (postfilter.hip), written against a memory policy so that the
// SAME text runs on LDS labels, on global labels and -- as plain C++ -- on the host (tools/spk_unionfind_check.cpp walks
// the tiles serially, shuffled and on threads under the address and undefined-behaviour sanitizers).
//
// The label invariant: labels only ever decrease, label[x] <= x at all times, label[x] == x defines a root.  Hence
//   * every walk of spk_find strictly descends and ends at a root (of that moment);
//   * every retry of spk_union strictly lowers `a`: it ends after at most `a` retries whatever the other threads do;
//   * nothing waits for another thread's progress: no flag, no ticket, no spin.
// Mem provides  int load(int i)  and  int fetch_min(int i, int v)  (returns the value before), both atomic at the scope
// at which the labels are shared.
#ifndef DCA_SPK_UNIONFIND_H
#define DCA_SPK_UNIONFIND_H

#if defined(__HIPCC__)
#define SPK_HD __host__ __device__ __forceinline__
#else
#define SPK_HD inline
#endif

// two ACTIVE 4-neighbours are joined iff |a - b| <= max_diff: the subtraction rounded to fp32, equality joins, symmetric
SPK_HD bool spk_joined(float a, float b, float max_diff) { return __builtin_fabsf(a - b) <= max_diff; }

// finite: not NaN and |v| < inf (a NaN fails the comparison)
SPK_HD bool spk_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

template <class Mem>
SPK_HD int spk_find(const Mem& m, int i) {
  for (int p = m.load(i); p != i; p = m.load(i)) i = p;      // p < i: label[i] <= i
  return i;
}

template <class Mem>
SPK_HD void spk_union(const Mem& m, int a, int b) {
  for (;;) {
    a = spk_find(m, a);
    b = spk_find(m, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = m.fetch_min(a, b);                       // hook the larger root under the smaller one
    if (old == a) return;                                    // a was still a root: done
    a = old;                                                 // label[a] was lowered meanwhile (old < a): go on from there
  }
}

// Boundary pair e of the merge launch over a rows x cols window cut into TH x TW tiles: the (tiles_x - 1) rows pairs across
// the vertical tile edges first (edge-major, top to bottom), then the (tiles_y - 1) cols pairs across the horizontal ones.
// Pixel a is the last column / row of its tile, b its neighbour in the next tile; labels are window indices r cols + c, < 0 for
// an inactive pixel (that never changes).  A pair is skipped when the pair before it along the same edge, inside the same
// two tiles, is joined across the edge AND joined to this pair on both sides: the tile-local pass has united a with a' and
// b with b' already, so the union would find equal roots -- a constant frame sends one union per tile edge, not one per
// edge pixel.  Val provides  float at(int r, int c).
template <int TH, int TW, class Mem, class Val>
SPK_HD void spk_merge_edge(const Mem& m, const Val& v, int e, int rows, int cols, int tiles_x, float max_diff) {
  const int nv = (tiles_x - 1) * rows;
  int ra, ca, rb, cb, rp, cp, rq, cq;                        // a, b and the pair before them (p beside a, q beside b)
  bool prev;
  if (e < nv) {
    const int edge = e / rows, r = e - edge * rows;
    ra = rb = r, ca = (edge + 1) * TW - 1, cb = ca + 1;
    prev = r % TH != 0, rp = rq = r - 1, cp = ca, cq = cb;
  } else {
    e -= nv;
    const int edge = e / cols, c = e - edge * cols;
    ca = cb = c, ra = (edge + 1) * TH - 1, rb = ra + 1;
    prev = c % TW != 0, cp = cq = c - 1, rp = ra, rq = rb;
  }
  const int ia = ra * cols + ca, ib = rb * cols + cb;
  if (m.load(ia) < 0 || m.load(ib) < 0) return;
  const float va = v.at(ra, ca), vb = v.at(rb, cb);
  if (!spk_joined(va, vb, max_diff)) return;
  if (prev && m.load(rp * cols + cp) >= 0 && m.load(rq * cols + cq) >= 0) {
    const float vp = v.at(rp, cp), vq = v.at(rq, cq);
    if (spk_joined(vp, vq, max_diff) && spk_joined(vp, va, max_diff) && spk_joined(vq, vb, max_diff)) return;
  }
  spk_union(m, ia, ib);
}

// the total order of the median: the bits b of a float as an unsigned key, -0.0 < +0.0, and back
SPK_HD unsigned spk_key(unsigned b) { return b ^ ((unsigned)((int)b >> 31) | 0x80000000u); }
SPK_HD unsigned spk_unkey(unsigned k) { return (k & 0x80000000u) ? k ^ 0x80000000u : ~k; }

#endif  // DCA_SPK_UNIONFIND_H
