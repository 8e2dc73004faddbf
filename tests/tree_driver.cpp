// Runs the device route's tree tables, per-cell result and per-goal path (csrc/vhp_tree.hpp: tree_build_tables, tree_cell,
// tree_goal_path) on the host.  Built by tests/test_tree_walk.py with the host compiler, once plain and once with the address and
// undefined-behaviour sanitizers: every buffer here has exactly the size the header asks for, so that a read or write past it is caught.
// stdin, binary, one record per table until end of file:
//   int32 nx, ny, n_pivots, cap (-1: no path buffer), n_goals (-1: every cell of the grid, row-major), then nx * ny uint32 labels
//   (0xFFFFFFFF = unlabelled), 2 * (n_pivots + 1) int32 pivot coordinates and 2 * n_goals int32 goal coordinates.
// stdout, one line per goal: status n_path, the length's bits in hex, 1 if every int of the path buffer beyond the points written is
// still kSentinel (all of it unless the status is 0), the length field's n_path and length bits for that cell (0 and 0 for a goal
// outside the grid, which has no cell), then the points written.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vhp_tree.hpp"

constexpr int32_t kSentinel = -777;

template <typename T>
static bool read_n(std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, stdin) == n;
}

static uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

int main() {
  int32_t h[5];
  while (std::fread(h, sizeof(int32_t), 5, stdin) == 5) {
    const int nx = h[0], ny = h[1], cap = h[3];
    const uint32_t n_pivots = (uint32_t)h[2];
    std::vector<uint32_t> label;
    std::vector<int32_t> pivots, goals;
    if (!read_n(label, (size_t)nx * ny) || !read_n(pivots, 2 * ((size_t)n_pivots + 1))) return 2;
    if (h[4] >= 0) {
      if (!read_n(goals, 2 * (size_t)h[4])) return 2;
    } else {
      for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) { goals.push_back(x); goals.push_back(y); }
    }
    std::vector<uint32_t> parent((size_t)n_pivots + 1), depth((size_t)n_pivots + 1);
    std::vector<double> cum((size_t)n_pivots + 1);
    vhp::tree_build_tables(label.data(), pivots.data(), n_pivots, nx, ny, parent.data(), depth.data(), cum.data());
    const size_t n_buf = cap >= 0 ? 2 * (size_t)cap : 0;
    std::unique_ptr<int32_t[]> path(new int32_t[n_buf]);   // (not null for cap = 0: a buffer without room, not "no buffer")
    for (size_t g = 0; g < goals.size() / 2; ++g) {
      const int x = goals[2 * g], y = goals[2 * g + 1];
      std::fill(path.get(), path.get() + n_buf, kSentinel);
      uint32_t n = 12345;
      double len = -2.0;
      const int st = vhp::tree_goal_path(label.data(), parent.data(), depth.data(), cum.data(), pivots.data(), n_pivots, nx, ny, x, y,
                                         cap >= 0 ? path.get() : nullptr, cap >= 0 ? (uint32_t)cap : 0u, &n, &len);
      const size_t written = st == vhp::kPathsOk && cap >= 0 ? 2 * (size_t)n : 0;
      const bool clean = std::all_of(path.get() + written, path.get() + n_buf, [](int32_t v) { return v == kSentinel; });
      uint32_t fn = 0;
      double flen = 0.0;
      if (x >= 0 && y >= 0 && x < nx && y < ny)
        vhp::tree_cell(label[(size_t)x + (size_t)y * nx], x, y, n_pivots, depth.data(), cum.data(), pivots.data(), &fn, &flen);
      std::printf("%d %u %016" PRIx64 " %d %u %016" PRIx64, st, n, bits_of(len), clean ? 1 : 0, fn, bits_of(flen));
      for (size_t k = 0; k < written; ++k) std::printf(" %d", path[k]);
      std::printf("\n");
    }
  }
  return 0;
}
