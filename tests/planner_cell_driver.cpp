// Runs one planner step's per-cell work (csrc/vhp_planner_cell.hpp: planner_unswept, eval_d_dev, planner_h, push_rank, key_less -- the
// functions the epilogue kernels call) on the host, over every cell of a grid, in the epilogue's order of operations: a cell the pivot
// does not sweep is skipped; fmax of the local value into the union; the cell is labelled if v >= thr and it is unlabelled; it is pushed
// if g >= thr; the pick is the arg-min of (h bits, rank) over the pushed cells.
// Built by tests/test_planner_cell_cpu.py with the host compiler, once plain and once with the address and undefined-behaviour
// sanitizers: every buffer here has exactly the size the step asks for.
// `planner_cell_driver step`: stdin, binary, one record per case until end of file:
//   int32 nx, ny, sx, sy, ex, ey, nb (the step's label: the pivot list holds nb + 1 pivots), float64 thr, then nx * ny float64 of the
//   local field, nx * ny float64 of the union before the step, nx * ny uint32 labels (0xFFFFFFFF = unlabelled), 2 * (nb + 1) int32 pivots.
// stdout, one line per case: pick x y (-1 -1: nothing pushed), its h bits in hex, its rank in hex, cells at the minimal h bits, cells
// pushed, then per cell a character (u: unswept, p: pushed, .: neither), the labels after the step and the union's bits after the step.
// `planner_cell_driver rank`: stdin int32 nx, ny per record; stdout one line per record: push_rank in hex for every pivot (row-major)
// and, inside a pivot, every cell (row-major).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vhp_planner_cell.hpp"
#include "vhp_planner_host.hpp"

constexpr uint32_t kUnlabelled32 = 0xffffffffu;

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

static int run_rank() {
  int32_t h[2];
  while (std::fread(h, sizeof(int32_t), 2, stdin) == 2) {
    const int nx = h[0], ny = h[1];
    if (nx <= 0 || ny <= 0) return 3;
    for (int sy = 0; sy < ny; ++sy)
      for (int sx = 0; sx < nx; ++sx)
        for (int y = 0; y < ny; ++y)
          for (int x = 0; x < nx; ++x) std::printf("%llx ", vhp::push_rank(nx, ny, sx, sy, x, y));
    std::printf("\n");
  }
  return 0;
}

static int run_step() {
  int32_t h[7];
  while (std::fread(h, sizeof(int32_t), 7, stdin) == 7) {
    const int nx = h[0], ny = h[1], sx = h[2], sy = h[3], ex = h[4], ey = h[5], nb = h[6];
    double thr;
    if (std::fread(&thr, sizeof(double), 1, stdin) != 1) return 2;
    if (nx <= 0 || ny <= 0 || nb < 0) return 3;
    const size_t cells = (size_t)nx * ny;
    std::vector<double> local, uni;
    std::vector<uint32_t> label;
    std::vector<int32_t> pivots;
    if (!read_n(local, cells) || !read_n(uni, cells) || !read_n(label, cells) || !read_n(pivots, 2 * ((size_t)nb + 1))) return 2;
    const double scale = vhp::planner_scale(nx, ny);
    vhp::PlannerKey best;
    best.h = ~0ull;
    best.rank = ~0ull;
    best.x = best.y = -1;
    std::string what(cells, '.');
    std::vector<unsigned long long> hs;
    for (size_t k = 0; k < cells; ++k) {
      const int y = (int)(k / (size_t)nx), x = (int)(k - (size_t)y * nx);
      if (vhp::planner_unswept(sx, sy, x, y)) { what[k] = 'u'; continue; }
      const double v = local[k];
      const double old = uni[k];
      const double g = std::fmax(v, old);
      uni[k] = g;
      if (g >= thr) {
        uint32_t lab = label[k];
        if (v >= thr && lab == kUnlabelled32) {
          lab = (uint32_t)nb;
          label[k] = lab;
        }
        if (lab > (uint32_t)nb) return 4;   // (a lit cell without a label: no state a solve leaves)
        const int px = pivots[2 * (size_t)lab], py = pivots[2 * (size_t)lab + 1];
        const double hh = vhp::planner_h(scale, g, vhp::eval_d_dev(x, y, ex, ey), vhp::eval_d_dev(x, y, px, py));
        vhp::PlannerKey c;
        c.h = bits_of(hh);
        c.rank = vhp::push_rank(nx, ny, sx, sy, x, y);
        c.x = x;
        c.y = y;
        if (vhp::key_less(c, best)) best = c;
        what[k] = 'p';
        hs.push_back(c.h);
      }
    }
    size_t tied = 0;
    for (unsigned long long v : hs) tied += v == best.h;
    std::printf("%d %d %llx %llx %zu %zu %s", best.x, best.y, best.h, best.rank, tied, hs.size(), what.c_str());
    for (size_t k = 0; k < cells; ++k) std::printf(" %" PRIx32, label[k]);
    for (size_t k = 0; k < cells; ++k) std::printf(" %" PRIx64, bits_of(uni[k]));
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "step")) return run_step();
  if (argc == 2 && !std::strcmp(argv[1], "rank")) return run_rank();
  return 1;
}
