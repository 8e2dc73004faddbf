// inflate_driver.cpp -- csrc/vhp_inflate.hpp on the CPU (tests/test_inflate_cpu.py builds it through tests/cpu_driver.py, plain and
// under the sanitizers): the footprints' half-width tables, and packed maps inflated word by word the way vhp_inflate_stack does it.
//   inflate_driver table
//       every disc p in 0 .. 4224 and every square and diamond p in 0 .. 64: the table against the shape's predicate, here, and one
//       line "shape p reach hw[0] .. hw[reach]" each on stdout; p = 4225 / 65, p = -1 and the shapes -1 and 3 must be refused.
//   inflate_driver words <packed maps file> <nx> <ny> <n_maps>
//       the file: per map the row-packed copy (ny lines of (nx + 63) / 64 + 2 words), then the column-packed one (nx lines of
//       (ny + 63) / 64 + 2), 64-bit words as the host stores them.  stdin: one footprint "shape p border" per line.  stdout: per
//       footprint, per map, the inflated row-packed words, then the column-packed ones.  Every output is also held, here, to the
//       definition evaluated cell by cell on the map's bits, and to the layout: pads 0, bits past a line's end 0.
// Exit 0: all held; 2: usage or input; 3: a check failed (what, on stderr).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vhp_inflate.hpp"

namespace {

bool in_footprint(int shape, int p, int dx, int dy) {
  const int ax = std::abs(dx), ay = std::abs(dy);
  return shape == 0 ? dx * dx + dy * dy <= p : shape == 1 ? std::max(ax, ay) <= p : ax + ay <= p;
}

int check_tables() {
  const int box = vhp::kMaxInflate + 2;  // (one cell past any valid footprint's reach, and one more)
  for (int shape = 0; shape <= 2; ++shape) {
    const int last = shape == 0 ? 4224 : 64;
    for (int p = 0; p <= last; ++p) {
      vhp::InflateTable t;
      std::memset(&t, 0x5a, sizeof t);
      if (!vhp::inflate_table(shape, p, &t)) { std::fprintf(stderr, "shape %d p %d refused\n", shape, p); return 3; }
      if (t.reach < 0 || t.reach > vhp::kMaxInflate) { std::fprintf(stderr, "shape %d p %d: reach %d\n", shape, p, t.reach); return 3; }
      for (int dy = 0; dy <= box; ++dy)
        for (int dx = 0; dx <= box; ++dx) {
          const bool by_table = dy <= t.reach && dx <= t.hw[dy];
          if (by_table != in_footprint(shape, p, dx, dy)) { std::fprintf(stderr, "shape %d p %d: (%d, %d)\n", shape, p, dx, dy); return 3; }
        }
      for (int d = t.reach + 1; d <= vhp::kMaxInflate; ++d)
        if (t.hw[d] != 0) { std::fprintf(stderr, "shape %d p %d: hw[%d] past the reach is %d\n", shape, p, d, t.hw[d]); return 3; }
      std::printf("%d %d %d", shape, p, t.reach);
      for (int d = 0; d <= t.reach; ++d) std::printf(" %d", t.hw[d]);
      std::printf("\n");
    }
    vhp::InflateTable t, before;
    std::memset(&t, 0x5a, sizeof t);
    before = t;
    for (int p : {last + 1, -1, 1 << 30})
      if (vhp::inflate_table(shape, p, &t) || std::memcmp(&t, &before, sizeof t) != 0) { std::fprintf(stderr, "shape %d p %d taken\n", shape, p); return 3; }
  }
  vhp::InflateTable t;
  if (vhp::inflate_table(-1, 1, &t) || vhp::inflate_table(3, 1, &t)) { std::fprintf(stderr, "unknown shape taken\n"); return 3; }
  return 0;
}

// One packed copy inflated: zeroed first (the memset of the device code: pads), then every data word from inflate_word.
std::vector<uint64_t> inflate_copy(const uint64_t* src, int lines, int cells, const vhp::InflateTable& t, bool border) {
  const int wpl = (cells + 63) / 64 + 2;
  std::vector<uint64_t> out((size_t)lines * wpl, 0);
  for (int j = 0; j < lines; ++j)
    for (int k = 0; k < wpl - 2; ++k) out[(size_t)j * wpl + 1 + k] = vhp::inflate_word(src, wpl, lines, cells, t, border, j, k);
  return out;
}

bool bit(const uint64_t* copy, int wpl, int line, int cell) { return (copy[(size_t)line * wpl + 1 + (cell >> 6)] >> (cell & 63)) & 1; }

// The inflated map by the definition, 1 = free: cell (x, y) is blocked exactly when some (x + dx, y + dy), (dx, dy) in `offs`, is
// blocked, a cell outside the grid being blocked only with `border`.  Either every cell looks for a blocked cell among its offsets
// -- far offsets first, where the border is, and stopping at the first find -- or, on a map with few blocked cells and a free
// outside, every blocked cell marks the cells that see it (the footprints are symmetric): the same statement, whichever is cheaper.
std::vector<uint8_t> by_definition(const std::vector<uint8_t>& free_in, int nx, int ny, const std::vector<std::pair<int, int>>& offs, bool border) {
  std::vector<uint8_t> out((size_t)nx * ny, 1);
  size_t n_blocked = 0;
  for (uint8_t f : free_in) n_blocked += !f;
  if (!border && n_blocked * 10 < free_in.size()) {
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        if (free_in[(size_t)y * nx + x]) continue;
        for (const auto& o : offs) {
          const int ox = x - o.first, oy = y - o.second;
          if (ox >= 0 && ox < nx && oy >= 0 && oy < ny) out[(size_t)oy * nx + ox] = 0;
        }
      }
    return out;
  }
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x)
      for (const auto& o : offs) {
        const int cx = x + o.first, cy = y + o.second;
        const bool inside = cx >= 0 && cx < nx && cy >= 0 && cy < ny;
        if (inside ? !free_in[(size_t)cy * nx + cx] : border) { out[(size_t)y * nx + x] = 0; break; }
      }
  return out;
}

// A packed copy against the cells it should hold (cell(line, c): 1 = free), the pads and the bits past the end
template <typename Cell>
bool copy_holds(const std::vector<uint64_t>& copy, int lines, int cells, Cell cell, const char* what) {
  const int wpl = (cells + 63) / 64 + 2;
  for (int j = 0; j < lines; ++j) {
    if (copy[(size_t)j * wpl] != 0 || copy[(size_t)j * wpl + wpl - 1] != 0) { std::fprintf(stderr, "%s: line %d: a pad is not 0\n", what, j); return false; }
    for (int c = 0; c < 64 * (wpl - 2); ++c) {
      const bool want = c < cells && cell(j, c);
      if (bit(copy.data(), wpl, j, c) != want) { std::fprintf(stderr, "%s: line %d cell %d of %d: %d, not %d\n", what, j, c, cells, !want, want); return false; }
    }
  }
  return true;
}

int run_words(const char* path, int nx, int ny, int n_maps) {
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
  int shape, p, border;
  while (std::scanf("%d %d %d", &shape, &p, &border) == 3) {
    vhp::InflateTable t;
    if (!vhp::inflate_table(shape, p, &t)) return 2;
    std::vector<std::pair<int, int>> offs;
    const int box = vhp::kMaxInflate + 1;
    for (int dy = -box; dy <= box; ++dy)
      for (int dx = -box; dx <= box; ++dx)
        if (in_footprint(shape, p, dx, dy)) offs.emplace_back(dx, dy);
    std::stable_sort(offs.begin(), offs.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) {
      return std::max(std::abs(a.first), std::abs(a.second)) > std::max(std::abs(b.first), std::abs(b.second));
    });
    for (int m = 0; m < n_maps; ++m) {
      const std::vector<uint64_t> r = inflate_copy(rows[m].data(), ny, nx, t, border != 0);
      const std::vector<uint64_t> c = inflate_copy(cols[m].data(), nx, ny, t, border != 0);
      const std::vector<uint8_t> want = by_definition(free_in[m], nx, ny, offs, border != 0);
      char what[128];
      std::snprintf(what, sizeof what, "map %d of %d x %d, shape %d p %d border %d, rows", m, nx, ny, shape, p, border);
      if (!copy_holds(r, ny, nx, [&](int y, int x) { return want[(size_t)y * nx + x] != 0; }, what)) return 3;
      std::snprintf(what, sizeof what, "map %d of %d x %d, shape %d p %d border %d, cols", m, nx, ny, shape, p, border);
      if (!copy_holds(c, nx, ny, [&](int x, int y) { return want[(size_t)y * nx + x] != 0; }, what)) return 3;
      std::fwrite(r.data(), 8, r.size(), stdout);
      std::fwrite(c.data(), 8, c.size(), stdout);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "table")) return check_tables();
  if (argc == 6 && !std::strcmp(argv[1], "words")) {
    const int nx = std::atoi(argv[3]), ny = std::atoi(argv[4]), n_maps = std::atoi(argv[5]);
    if (nx < 1 || ny < 1 || n_maps < 1) return 2;
    return run_words(argv[2], nx, ny, n_maps);
  }
  std::fprintf(stderr, "usage: inflate_driver table | inflate_driver words <packed maps file> <nx> <ny> <n_maps>   (footprints \"shape p border\" on stdin)\n");
  return 2;
}
