// Host check of the speckle filter's union-find (csrc/spk_unionfind.h, the text the kernels of csrc/postfilter.hip
// compile): the four launches restated in plain C++ over the SAME find / union / merge-edge functions, with the tiles and
// the pairs walked (a) in order, (b) in a shuffled order and (c) on four threads at once, each compared with a flood fill.
// A wrong union-find hangs rather than fails, so this runs before anything goes to a GPU:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -D__HIP_PLATFORM_AMD__ \
//       -I <rocm>/include -I <package>/csrc -I include tools/spk_unionfind_check.cpp -o spk_check && ./spk_check
// (include/dca_hip.h, read for the tile size, includes the HIP runtime's API header; no device is touched.)
// Exit status 0 and "ok" when every case agrees.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "dca_hip.h"
#include "spk_unionfind.h"

namespace {

constexpr int TH = DCA_SPK_TILE_H, TW = DCA_SPK_TILE_W, PIX = TH * TW;

struct Labels {                                              // Mem of spk_unionfind.h on host memory
  int* l;
  int load(int i) const { return __atomic_load_n(l + i, __ATOMIC_RELAXED); }
  void store(int i, int v) const { __atomic_store_n(l + i, v, __ATOMIC_RELAXED); }
  int fetch_min(int i, int v) const {
    int old = load(i);
    while (old > v && !__atomic_compare_exchange_n(l + i, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
  }
};

struct Values {
  const float* d;
  int cols;
  float at(int r, int c) const { return d[(long)r * cols + c]; }
};

struct Case {
  const char* name;
  int rows, cols;
  std::vector<float> d;
  std::vector<char> masked;
  float max_diff;
};

std::vector<int> order(int n, std::mt19937* rng) {
  std::vector<int> o(n);
  for (int i = 0; i < n; ++i) o[i] = i;
  if (rng) std::shuffle(o.begin(), o.end(), *rng);
  return o;
}

// launch 1 for one tile: the phases of spk_local_kernel, the pixels of a phase in the order `o`
void local_tile(const Case& k, int ty0, int tx0, const std::vector<int>& o, int* label, int* count) {
  float val[PIX];
  int lab[PIX], cnt[PIX], root[PIX];
  unsigned char join[PIX];
  const Labels L = {lab};
  for (int i = 0; i < PIX; ++i) {
    const int r = ty0 + i / TW, c = tx0 + i % TW;
    const bool in = r < k.rows && c < k.cols;
    val[i] = in ? k.d[r * k.cols + c] : 0.f;
    lab[i] = in && spk_finite(val[i]) && !k.masked[r * k.cols + c] ? i : -1;
    cnt[i] = 0;
  }
  for (int i = 0; i < PIX; ++i) {
    unsigned j = 0;
    if (lab[i] >= 0) {
      if (i % TW > 0 && lab[i - 1] >= 0 && spk_joined(val[i], val[i - 1], k.max_diff)) j |= 1u;
      if (i >= TW && lab[i - TW] >= 0 && spk_joined(val[i], val[i - TW], k.max_diff)) j |= 2u;
    }
    join[i] = (unsigned char)j;
  }
  for (int i = 0; i < PIX; ++i)
    if (join[i] & 1u) lab[i] = i - 1;
  for (int n = 0; n < 6; ++n)
    for (int i : o) {
      const int p = L.load(i);
      if (p >= 0 && p != i) L.store(i, L.load(p));
    }
  for (int i = 0; i < PIX; ++i)
    if ((join[i] & 1u) && lab[i] >= 0 && (join[lab[i]] & 1u)) { std::printf("%s: run not flattened\n", k.name); std::exit(1); }
  for (int i : o)
    if ((join[i] & 2u) && !((join[i] & 1u) && (join[i - 1] & 2u) && (join[i - TW] & 1u))) spk_union(L, i, i - TW);
  for (int i : o) {
    root[i] = lab[i] >= 0 ? spk_find(L, i) : -1;
    if (root[i] >= 0) ++cnt[root[i]];
  }
  for (int i = 0; i < PIX; ++i) {
    const int r = ty0 + i / TW, c = tx0 + i % TW;
    if (r < k.rows && c < k.cols) {
      label[r * k.cols + c] = root[i] >= 0 ? (ty0 + root[i] / TW) * k.cols + tx0 + root[i] % TW : -1;
      count[r * k.cols + c] = root[i] == i ? cnt[i] : 0;
    }
  }
}

void count_pixel(const Labels& G, int* cnt, int i) {         // spk_count_kernel
  if (G.load(i) == i) return;
  const int c = cnt[i];
  if (c <= 0) return;
  const int r = spk_find(G, i);
  __atomic_fetch_add(cnt + r, c, __ATOMIC_RELAXED);
  G.store(i, r);
}

// mode 0: in order; 1: shuffled; 2: four threads, shuffled
std::vector<int> run(const Case& k, int mode, std::mt19937& rng) {
  const int n = k.rows * k.cols, tiles_x = (k.cols + TW - 1) / TW, tiles_y = (k.rows + TH - 1) / TH;
  std::vector<int> label(n, 12345), count(n, -777);          // garbage: the launches must initialise everything
  for (int t : order(tiles_x * tiles_y, mode ? &rng : nullptr))
    local_tile(k, (t / tiles_x) * TH, (t % tiles_x) * TW, order(PIX, mode ? &rng : nullptr), label.data(), count.data());
  for (int i = 0; i < n; ++i)
    if (label[i] > i) { std::printf("%s: label[%d] = %d > index after launch 1\n", k.name, i, label[i]); std::exit(1); }
  const Labels G = {label.data()};
  const Values V = {k.d.data(), k.cols};
  const int pairs = (tiles_x - 1) * k.rows + (tiles_y - 1) * k.cols;
  auto in_threads = [&](const std::vector<int>& o, const std::function<void(int)>& f) {
    if (mode < 2) {
      for (int e : o) f(e);
      return;
    }
    std::vector<std::thread> th;
    for (int w = 0; w < 4; ++w)
      th.emplace_back([&, w] { for (size_t j = w; j < o.size(); j += 4) f(o[j]); });
    for (auto& x : th) x.join();
  };
  in_threads(order(pairs, mode ? &rng : nullptr),
             [&](int e) { spk_merge_edge<TH, TW>(G, V, e, k.rows, k.cols, tiles_x, k.max_diff); });
  for (int i = 0; i < n; ++i)
    if (label[i] > i) { std::printf("%s: label[%d] = %d > index after launch 2\n", k.name, i, label[i]); std::exit(1); }
  in_threads(order(n, mode ? &rng : nullptr), [&](int i) { count_pixel(G, count.data(), i); });
  std::vector<int> size(n, 0);
  for (int i = 0; i < n; ++i) {
    int r = label[i];
    if (r < 0) continue;
    int hops = 0;
    for (int p = label[r]; p != r; p = label[r]) r = p, ++hops;
    if (hops > 1) { std::printf("%s: %d links from a tile-local root in launch 4\n", k.name, hops); std::exit(1); }
    size[i] = count[r];
  }
  return size;
}

std::vector<int> flood(const Case& k) {
  const int n = k.rows * k.cols;
  std::vector<int> size(n, 0), comp(n, -1), stack;
  for (int s = 0; s < n; ++s) {
    if (comp[s] >= 0 || !spk_finite(k.d[s]) || k.masked[s]) continue;
    std::vector<int> members;
    stack.assign(1, s);
    comp[s] = s;
    while (!stack.empty()) {
      const int i = stack.back(), r = i / k.cols, c = i % k.cols;
      stack.pop_back();
      members.push_back(i);
      const int nb[4] = {c > 0 ? i - 1 : -1, c + 1 < k.cols ? i + 1 : -1, r > 0 ? i - k.cols : -1, r + 1 < k.rows ? i + k.cols : -1};
      for (int j : nb)
        if (j >= 0 && comp[j] < 0 && spk_finite(k.d[j]) && !k.masked[j] && spk_joined(k.d[i], k.d[j], k.max_diff)) {
          comp[j] = s;
          stack.push_back(j);
        }
    }
    for (int i : members) size[i] = (int)members.size();
  }
  return size;
}

Case make(const char* name, int rows, int cols, float max_diff, const std::function<float(int, int)>& f) {
  Case k = {name, rows, cols, std::vector<float>((size_t)rows * cols), std::vector<char>((size_t)rows * cols, 0), max_diff};
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) k.d[r * cols + c] = f(r, c);
  return k;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  std::vector<Case> cases;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (auto hw : {std::pair<int, int>{37, 83}, {70, 150}, {5, 7}, {1, 1}, {1, TW + 1}, {TH + 1, 1}, {384, 1248}}) {
    Case k = make("scene", hw.first, hw.second, 1.f, [&](int r, int c) {
      float v = 20.f + 0.05f * c + 0.02f * r + (c >= hw.second / 2 ? 7.3f : 0.f);
      if (rng() % 100 < 3) v += 3.f + (rng() % 2700) / 100.f;
      if (rng() % 200 == 0) v = rng() % 3 == 0 ? nan : rng() % 2 ? inf : -inf;
      return v;
    });
    for (auto& m : k.masked) m = rng() % 50 == 0;
    cases.push_back(k);
  }
  cases.push_back(make("snake", 2 * TH + 3, 2 * TW + 5, 1.f, [](int r, int c) {
    const int W = 2 * TW + 5;
    return r % 2 == 0 || (r % 4 == 1 ? c == W - 1 : c == 0) ? 10.f : 50.f;
  }));
  cases.push_back(make("snake at the frame's size", 384, 1248, 1.f, [](int r, int c) {
    return r % 2 == 0 || (r % 4 == 1 ? c == 1247 : c == 0) ? 10.f : 50.f;
  }));
  cases.push_back(make("constant", 3 * TH, 3 * TW + 1, 0.f, [](int, int) { return 4.f; }));
  cases.push_back(make("constant at the frame's size", 384, 1248, 0.f, [](int, int) { return -0.f; }));
  cases.push_back(make("checkerboard", 2 * TH + 1, 2 * TW + 1, 1.f, [](int r, int c) { return (r + c) % 2 ? 10.f : 0.f; }));
  cases.push_back(make("ramp, chained", TH + 3, 2 * TW + 2, 1.f, [](int, int c) { return 0.75f * c; }));
  cases.push_back(make("ramp, columns", TH + 3, 2 * TW + 2, 1.f, [](int, int c) { return 1.25f * c; }));
  cases.push_back(make("ramp, equality", TH + 3, 2 * TW + 2, 0.5f, [](int r, int c) { return 0.5f * ((r + c) % 5); }));
  cases.push_back(make("random", 3 * TH + 2, 3 * TW + 7, 1.f, [&](int, int) { return (float)(rng() % 4); }));
  for (const Case& k : cases) {
    const std::vector<int> want = flood(k);
    for (int mode = 0; mode < 3; ++mode)
      for (int rep = 0; rep < (mode ? 3 : 1); ++rep)
        if (run(k, mode, rng) != want) {
          std::printf("%s (%d x %d), mode %d: sizes differ from the flood fill\n", k.name, k.rows, k.cols, mode);
          return 1;
        }
    std::printf("%-28s %4d x %4d  agrees in order, shuffled and on four threads\n", k.name, k.rows, k.cols);
  }
  std::printf("ok\n");
  return 0;
}
