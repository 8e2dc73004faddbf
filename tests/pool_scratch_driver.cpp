// Holds the sizes the pool sweep's launcher gives the scratch of a launch (csrc/vhp_pool_scratch.hpp) against what the sweep asks of
// it (csrc/vhp_pool.hpp UnitGeo), on the host.  Built by tests/test_pool_scratch_bound.py with the host compiler and -DVHP_SIM, once
// plain and once with the address and undefined-behaviour sanitizers.
// stdin, one request per line:
//   lines NX NY all            every cell of the grid as a source
//   lines NX NY sampled        every 7th cell in row-major order, and every cell with a coordinate in {0, 1, 15, 16, 63, 64, n/2, n-2, n-1}
//   lines NX NY list N x0 y0 x1 y1 ...   the N sources given (one outside the grid needs nothing, as in vhp_pool_order)
//   sizes N NX NY              the scratch of a launch of N sources
// stdout, one line per request:
//   lines: bound need sx sy units sources -- line_blocks_per_source(NX, NY); the largest sum over a source's 8 units of
//          UnitGeo::line_blocks() and the first source that attains it; the units with line_blocks() > 0 over all the sources; the sources
//   sizes: head_bytes(N), the bytes of the layout launch_pool_t carves from it (pull counter, records, order, line bases), diag_bytes(N, NX, NY),
//          diag_stride_of(NX, NY)
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "vhp_pool.hpp"
#include "vhp_pool_scratch.hpp"

namespace {

struct Worst {
  long long need = -1, units = 0, sources = 0;
  int sx = -1, sy = -1;
  void add(int nx, int ny, int sx_, int sy_) {
    ++sources;
    long long sum = 0;
    if (!(sx_ < 0 || sy_ < 0 || sx_ >= nx || sy_ >= ny)) {
      for (int qo = 0; qo < vhp::pool::kUnits; ++qo) {
        vhp::pool::UnitGeo g;
        g.init(nx, ny, qo, sx_, sy_);
        const int nb = g.line_blocks();
        sum += nb;
        units += nb > 0;
      }
    }
    if (sum > need) { need = sum; sx = sx_; sy = sy_; }
  }
};

std::vector<int> special(int n) {
  std::set<int> s;
  for (int v : {0, 1, 15, 16, 63, 64, n / 2, n - 2, n - 1})
    if (v >= 0 && v < n) s.insert(v);
  return std::vector<int>(s.begin(), s.end());
}

}  // namespace

int main() {
  char what[16], mode[16];
  while (std::scanf("%15s", what) == 1) {
    if (!std::strcmp(what, "sizes")) {
      int n, nx, ny;
      if (std::scanf("%d %d %d", &n, &nx, &ny) != 3) return 2;
      const size_t layout = sizeof(int) * ((size_t)vhp::kQueueInts + (size_t)(4 + 1 + 1) * vhp::pool::kUnits * (size_t)n);
      std::printf("%zu %zu %zu %d\n", vhp::head_bytes(n), layout, vhp::diag_bytes(n, nx, ny), vhp::diag_stride_of(nx, ny));
      continue;
    }
    int nx, ny;
    if (std::strcmp(what, "lines") || std::scanf("%d %d %15s", &nx, &ny, mode) != 3 || nx < 1 || ny < 1) return 2;
    Worst w;
    if (!std::strcmp(mode, "all")) {
      for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) w.add(nx, ny, x, y);
    } else if (!std::strcmp(mode, "sampled")) {
      for (long long c = 0; c < (long long)nx * ny; c += 7) w.add(nx, ny, (int)(c % nx), (int)(c / nx));
      for (int x : special(nx))
        for (int y = 0; y < ny; ++y) w.add(nx, ny, x, y);
      for (int y : special(ny))
        for (int x = 0; x < nx; ++x) w.add(nx, ny, x, y);
    } else if (!std::strcmp(mode, "list")) {
      int n;
      if (std::scanf("%d", &n) != 1 || n < 0) return 2;
      for (int k = 0; k < n; ++k) {
        int x, y;
        if (std::scanf("%d %d", &x, &y) != 2) return 2;
        w.add(nx, ny, x, y);
      }
    } else {
      return 2;
    }
    std::printf("%lld %lld %d %d %lld %lld\n", vhp::line_blocks_per_source(nx, ny), w.need, w.sx, w.sy, w.units, w.sources);
  }
  return 0;
}
