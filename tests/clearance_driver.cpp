// clearance_driver.cpp -- csrc/vhp_clearance.hpp on the CPU (tests/test_clearance_cpu.py builds it through tests/cpu_driver.py, plain
// and under the sanitizers): the clearance of every cell of packed maps, the way vhp_clearance_stack combines it.
//   clearance_driver refuse
//       the p_max that vhp_map_clearance must refuse -- -1, 4225 for a disc, 65 for a square or a diamond, an unknown shape -- are
//       refused by the check it reuses (inflate_table), the last valid ones are taken, and clearance_reach is their reach.
//   clearance_driver cells <packed maps file> <nx> <ny> <n_maps>
//       the file: per map the row-packed copy (ny lines of (nx + 63) / 64 + 2 words), then the column-packed one (nx lines of
//       (ny + 63) / 64 + 2), 64-bit words as the host stores them.  stdin: one "shape p_max border" per line.  stdout: per line of
//       stdin, per map, the field from the row-packed copy (uint16 [ny][nx]), then the one from the column-packed copy with x and y
//       exchanged (uint16 [nx][ny]).  Every value is also held, here, to the definition evaluated cell by cell on the map's bits.
// Exit 0: all held; 2: usage or input; 3: a check failed (what, on stderr).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vhp_clearance.hpp"

namespace {

int metric(int shape, int dx, int dy) {
  const int ax = std::abs(dx), ay = std::abs(dy);
  return shape == 0 ? dx * dx + dy * dy : shape == 1 ? std::max(ax, ay) : ax + ay;
}

int check_refusals() {
  for (int shape = 0; shape <= 2; ++shape) {
    const int last = shape == 0 ? 4224 : 64;
    vhp::InflateTable t;
    for (int p : {-1, last + 1, 1 << 30})
      if (vhp::inflate_table(shape, p, &t)) { std::fprintf(stderr, "shape %d p_max %d taken\n", shape, p); return 3; }
    for (int p = 0; p <= last; ++p) {
      if (!vhp::inflate_table(shape, p, &t)) { std::fprintf(stderr, "shape %d p_max %d refused\n", shape, p); return 3; }
      if (vhp::clearance_reach(shape, p) != t.reach) { std::fprintf(stderr, "shape %d p_max %d: reach %d, not %d\n", shape, p, vhp::clearance_reach(shape, p), t.reach); return 3; }
      // every metric value a valid field can hold lies below the far value and comes from a g below the "none" byte
      if (p >= (int)vhp::kClearanceFar || t.reach >= vhp::kClearanceNone || vhp::clearance_metric(shape, vhp::kClearanceNone, 0) <= p) return 3;
    }
  }
  vhp::InflateTable t;
  if (vhp::inflate_table(-1, 1, &t) || vhp::inflate_table(3, 1, &t)) { std::fprintf(stderr, "unknown shape taken\n"); return 3; }
  return 0;
}

struct Offset {
  int dx, dy, m;
};

bool bit(const uint64_t* copy, int wpl, int line, int cell) { return (copy[(size_t)line * wpl + 1 + (cell >> 6)] >> (cell & 63)) & 1; }

// The field by the definition: the smallest m(dx, dy) <= p_max over the blocked cells (x + dx, y + dy), a cell outside the grid
// being blocked only with `border`.  `offs` holds every offset with m <= p_max in rising order of m.  Either every cell takes the
// first offset that finds a blocked cell, or, on a map with few blocked cells and a free outside, every blocked cell lowers the
// cells that see it (the metrics are symmetric): the same statement, whichever is cheaper.
std::vector<uint16_t> by_definition(const std::vector<uint8_t>& free_in, int nx, int ny, const std::vector<Offset>& offs, bool border) {
  std::vector<uint16_t> out((size_t)nx * ny, (uint16_t)vhp::kClearanceFar);
  size_t n_blocked = 0;
  for (uint8_t f : free_in) n_blocked += !f;
  if (!border && n_blocked * 10 < free_in.size()) {
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        if (free_in[(size_t)y * nx + x]) continue;
        for (const Offset& o : offs) {
          const int ox = x - o.dx, oy = y - o.dy;
          if (ox >= 0 && ox < nx && oy >= 0 && oy < ny && o.m < out[(size_t)oy * nx + ox]) out[(size_t)oy * nx + ox] = (uint16_t)o.m;
        }
      }
    return out;
  }
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x)
      for (const Offset& o : offs) {
        const int cx = x + o.dx, cy = y + o.dy;
        const bool inside = cx >= 0 && cx < nx && cy >= 0 && cy < ny;
        if (inside ? !free_in[(size_t)cy * nx + cx] : border) { out[(size_t)y * nx + x] = (uint16_t)o.m; break; }
      }
  return out;
}

int run_cells(const char* path, int nx, int ny, int n_maps) {
  const int wpr = (nx + 63) / 64 + 2, wpc = (ny + 63) / 64 + 2;
  const size_t row_words = (size_t)ny * wpr, col_words = (size_t)nx * wpc;
  // exactly the words of each copy, so that a read past either one is a read past an allocation
  std::vector<std::vector<uint64_t>> rows(n_maps), cols(n_maps);
  std::vector<std::vector<uint8_t>> free_in(n_maps);
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  for (int m = 0; m < n_maps; ++m) {
    rows[m].resize(row_words);
    cols[m].resize(col_words);
    if (std::fread(rows[m].data(), 8, row_words, f) != row_words || std::fread(cols[m].data(), 8, col_words, f) != col_words) return 2;
    free_in[m].resize((size_t)nx * ny);
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        free_in[m][(size_t)y * nx + x] = bit(rows[m].data(), wpr, y, x);
        if (bit(cols[m].data(), wpc, x, y) != bit(rows[m].data(), wpr, y, x)) { std::fprintf(stderr, "map %d: the two copies differ\n", m); return 2; }
      }
  }
  std::fclose(f);
  int shape, p_max, border;
  std::vector<uint16_t> by_rows((size_t)nx * ny), by_cols((size_t)nx * ny);
  while (std::scanf("%d %d %d", &shape, &p_max, &border) == 3) {
    vhp::InflateTable t;
    if (!vhp::inflate_table(shape, p_max, &t)) return 2;
    std::vector<Offset> offs;
    const int box = vhp::kMaxInflate + 1;
    for (int dy = -box; dy <= box; ++dy)
      for (int dx = -box; dx <= box; ++dx)
        if (metric(shape, dx, dy) <= p_max) offs.push_back({dx, dy, metric(shape, dx, dy)});
    std::stable_sort(offs.begin(), offs.end(), [](const Offset& a, const Offset& b) { return a.m < b.m; });
    for (int m = 0; m < n_maps; ++m) {
      const std::vector<uint16_t> want = by_definition(free_in[m], nx, ny, offs, border != 0);
      for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
          const unsigned r = vhp::clearance_cell(rows[m].data(), wpr, ny, nx, shape, p_max, border != 0, x, y);
          const unsigned c = vhp::clearance_cell(cols[m].data(), wpc, nx, ny, shape, p_max, border != 0, y, x);
          by_rows[(size_t)y * nx + x] = (uint16_t)r;
          by_cols[(size_t)x * ny + y] = (uint16_t)c;
          if (r != want[(size_t)y * nx + x] || c != r) {
            std::fprintf(stderr, "map %d of %d x %d, shape %d p_max %d border %d, cell (%d, %d): rows %u, cols %u, the definition %u\n", m, nx, ny, shape,
                         p_max, border, x, y, r, c, (unsigned)want[(size_t)y * nx + x]);
            return 3;
          }
        }
      std::fwrite(by_rows.data(), 2, by_rows.size(), stdout);
      std::fwrite(by_cols.data(), 2, by_cols.size(), stdout);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "refuse")) return check_refusals();
  if (argc == 6 && !std::strcmp(argv[1], "cells")) {
    const int nx = std::atoi(argv[3]), ny = std::atoi(argv[4]), n_maps = std::atoi(argv[5]);
    if (nx < 1 || ny < 1 || n_maps < 1) return 2;
    return run_cells(argv[2], nx, ny, n_maps);
  }
  std::fprintf(stderr, "usage: clearance_driver refuse | clearance_driver cells <packed maps file> <nx> <ny> <n_maps>   (\"shape p_max border\" on stdin)\n");
  return 2;
}
