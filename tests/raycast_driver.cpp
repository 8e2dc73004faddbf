// raycast_driver.cpp -- csrc/vhp_raycast.hpp on the CPU (tests/test_raycast_cpu.py builds it through tests/cpu_driver.py, plain and
// under the sanitizers): the ray walk over maps packed on the host, the launch plan's coverage, and the step count of a ray.
//   raycast_driver fields <map file> <nx> <ny>      sources "x y" per line on stdin; the fields, one byte per cell, on stdout
//   raycast_driver plan <cells> <n_src>             prints "tiles grid_y"; exit 1 unless every (tile, source) pair is taken exactly once
//   raycast_driver steps <max_side> | steps-of <dx> prints the rays checked; exit 1 where a ray differs from the reference's loop
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vhp_raycast.hpp"

namespace {

// The layout of vhp_pack_rows_stack / vhp_pack_cols_stack: wpr = ceil(nx / 64) + 2 words a row, the first and the last a zero pad.
struct HostMaps {
  int nx, ny, wpr, wpc;
  std::vector<uint64_t> rows, cols;
  HostMaps(const std::vector<uint8_t>& occ, int nx_, int ny_) : nx(nx_), ny(ny_), wpr((nx_ + 63) / 64 + 2), wpc((ny_ + 63) / 64 + 2) {
    rows.assign((size_t)ny * wpr, 0);
    cols.assign((size_t)nx * wpc, 0);
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x)
        if (occ[(size_t)y * nx + x] != 0) {
          rows[(size_t)y * wpr + 1 + (x >> 6)] |= (uint64_t)1 << (x & 63);
          cols[(size_t)x * wpc + 1 + (y >> 6)] |= (uint64_t)1 << (y & 63);
        }
  }
  vhp::PackedOcc packed() const { return {rows.data(), cols.data(), wpr, wpc}; }
};

int fields(const char* path, int nx, int ny) {
  std::vector<uint8_t> occ((size_t)nx * ny);
  FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(occ.data(), 1, occ.size(), f) != occ.size()) return 2;
  std::fclose(f);
  const HostMaps m(occ, nx, ny);
  const vhp::PackedOcc p = m.packed();
  std::vector<uint8_t> out(occ.size());
  int sx, sy;
  while (std::scanf("%d %d", &sx, &sy) == 2) {
    if (sx < 0 || sy < 0 || sx >= nx || sy >= ny) return 2;
    std::fill(out.begin(), out.end(), 1);  // what the kernels do: ones, then only zeros
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        int hx, hy;
        if (vhp::ray_walk(p, sx, sy, x, y, &hx, &hy)) {
          if (hx < 0 || hy < 0 || hx >= nx || hy >= ny) return 3;
          out[(size_t)hy * nx + hx] = 0;
          out[(size_t)y * nx + x] = 0;
        }
      }
    std::fwrite(out.data(), 1, out.size(), stdout);
  }
  return 0;
}

int plan(long long cells, int n_src) {
  const vhp::RaycastPlan p = vhp::plan_raycast(cells, n_src);
  std::printf("%u %u\n", p.tiles, p.grid_y);
  if (p.block != (unsigned)vhp::kRaycastBlock || p.grid_y > 65535u) return 1;
  if ((long long)p.tiles * p.block < cells || (long long)(p.tiles - 1) * p.block >= cells) return 1;  // the last tile holds a cell
  if ((n_src == 0) != (p.grid_y == 0)) return 1;
  std::vector<uint8_t> taken((size_t)p.tiles * n_src, 0);
  for (unsigned by = 0; by < p.grid_y; ++by)
    for (unsigned bx = 0; bx < p.tiles; ++bx)
      vhp::raycast_for_sources(by, p.grid_y, n_src, [&](int s) {
        if (s < 0 || s >= n_src || taken[(size_t)bx * n_src + s] == 255) std::exit(1);
        ++taken[(size_t)bx * n_src + s];
      });
  for (uint8_t t : taken)
    if (t != 1) return 1;
  return 0;
}

// The reference's loop (solver.cpp:267-290) from (x0, y0) to (x1, y1) beside ray_begin / ray_step: the same cells in the same order,
// exactly max(dx, dy) iterations, the major coordinate moved by one in each, the target reached.
bool same_as_reference(int x0, int y0, int x1, int y1) {
  vhp::Ray r = vhp::ray_begin(x0, y0, x1, y1);
  const int dx = std::abs(x1 - x0), dy = std::abs(y1 - y0);
  const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
  if (r.n != (dx > dy ? dx : dy)) return false;
  int err = dx - dy, k = 0;
  while (x0 != x1 || y0 != y1) {
    if (k >= r.n || r.x() != x0 || r.y() != y0) return false;
    const int e2 = 2 * err;
    if (e2 > -dy) { err -= dy; x0 += sx; }
    if (e2 < dx) { err += dx; y0 += sy; }
    const int a = r.a;
    vhp::ray_step(r);
    if (r.a != a + r.sa) return false;
    ++k;
  }
  return k == r.n && r.x() == x1 && r.y() == y1;
}

// both orientations of (dx, dy), each in its four directions
bool check_delta(int dx, int dy, long long* n) {
  for (int swap = 0; swap < 2; ++swap) {
    const int w = swap ? dy : dx, h = swap ? dx : dy;
    const int ends[4][4] = {{0, 0, w, h}, {w, h, 0, 0}, {0, h, w, 0}, {w, 0, 0, h}};
    for (const auto& e : ends) {
      if (!same_as_reference(e[0], e[1], e[2], e[3])) {
        std::printf("differs: (%d, %d) -> (%d, %d)\n", e[0], e[1], e[2], e[3]);
        return false;
      }
      ++*n;
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fields" && argc == 5) return fields(argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
  if (mode == "plan" && argc == 4) return plan(std::atoll(argv[2]), std::atoi(argv[3]));
  if ((mode == "steps" || mode == "steps-of") && argc == 3) {
    const int v = std::atoi(argv[2]);
    long long n = 0;
    if (mode == "steps") {  // every dx >= dy up to v (check_delta takes the other orientation along)
      for (int dx = 0; dx <= v; ++dx)
        for (int dy = 0; dy <= dx; ++dy)
          if (!check_delta(dx, dy, &n)) return 1;
    } else {
      for (int dy = 0; dy <= v; ++dy)
        if (!check_delta(v, dy, &n)) return 1;
    }
    std::printf("%lld\n", n);
    return 0;
  }
  std::fprintf(stderr, "usage: raycast_driver fields <map> <nx> <ny> | plan <cells> <n_src> | steps <max_side> | steps-of <dx>\n");
  return 2;
}
