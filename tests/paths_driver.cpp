// Runs the device route's path reconstruction (csrc/vhp_paths.hpp: paths_parent_entry for every pivot, then paths_walk) on the host.
// Built by tests/test_paths_walk.py with the host compiler, once plain and once with the address and undefined-behaviour sanitizers:
// every buffer here has exactly the size the header asks for, so that a read or write past it is caught.
// stdin, binary, one record per case until end of file:
//   int32 nx, ny, n_pivots, end_x, end_y, cap (-1: no path buffer), then nx * ny uint32 labels (0xFFFFFFFF = unlabelled) and
//   2 * (n_pivots + 1) int32 pivot coordinates.
// stdout, one line per case: status n_path, the length's bits in hex, then the whole path buffer (cap points; it starts out as
// kSentinel everywhere).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vhp_paths.hpp"

constexpr int32_t kSentinel = -777;

template <typename T>
static bool read_n(std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, stdin) == n;
}

int main() {
  int32_t h[6];
  while (std::fread(h, sizeof(int32_t), 6, stdin) == 6) {
    const int nx = h[0], ny = h[1], end_x = h[3], end_y = h[4];
    const uint32_t n_pivots = (uint32_t)h[2];
    std::vector<uint32_t> label;
    std::vector<int32_t> pivots;
    if (!read_n(label, (size_t)nx * ny) || !read_n(pivots, 2 * ((size_t)n_pivots + 1))) return 2;
    if (end_x < 0 || end_y < 0 || end_x >= nx || end_y >= ny) return 3;   // (the solves validate the end before anything runs)
    std::vector<uint32_t> parent((size_t)n_pivots + 1);
    for (uint32_t k = 0; k <= n_pivots; ++k) parent[k] = vhp::paths_parent_entry(label.data(), pivots.data(), k, nx, ny);
    std::vector<int32_t> rev(2 * ((size_t)n_pivots + 3));
    const size_t n_buf = h[5] >= 0 ? 2 * (size_t)h[5] : 0;
    std::unique_ptr<int32_t[]> path(new int32_t[n_buf]);   // (not null for cap = 0: a buffer without room, not "no buffer")
    std::fill(path.get(), path.get() + n_buf, kSentinel);
    uint32_t n = 12345;
    double len = -1.0;
    const int st = vhp::paths_walk(label[(size_t)end_x + (size_t)end_y * nx], parent.data(), pivots.data(), n_pivots, end_x, end_y, rev.data(),
                                   h[5] >= 0 ? path.get() : nullptr, h[5] >= 0 ? (uint32_t)h[5] : 0u, &n, &len);
    uint64_t bits;
    std::memcpy(&bits, &len, 8);
    std::printf("%d %u %016" PRIx64, st, n, bits);
    for (size_t k = 0; k < n_buf; ++k) std::printf(" %d", path[k]);
    std::printf("\n");
  }
  return 0;
}
