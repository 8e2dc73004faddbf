// window_driver.cpp -- csrc/vhp_window.hpp on the CPU (tests/test_window_cut_cpu.py builds it through tests/cpu_driver.py, plain and
// under the sanitizers): windows of a packed map, cut word by word the way vhp_cut_rows_stack / vhp_cut_cols_stack cut them.
//   window_driver <packed map file> <nx> <ny>     the file: the row-packed copy (ny lines of (nx + 63) / 64 + 2 words), then the
//                                                 column-packed one (nx lines of (ny + 63) / 64 + 2), 64-bit words as the host stores them
//   stdin: one window "w h ox oy" per line; stdout: per window its h * wpr row-packed words, then its w * wpc column-packed ones
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vhp_window.hpp"

namespace {

// One copy of a window: `lines` lines of `len` cells from line o_line, cell o_cell on, of a copy of src_lines lines of src_len cells.
// Zeroed first (the memset of the device code: pads), then every data word from window_word.
std::vector<uint64_t> cut(const uint64_t* src, int src_lines, int src_len, int o_line, int o_cell, int lines, int len) {
  const int src_wpl = (src_len + 63) / 64 + 2, wpl = (len + 63) / 64 + 2;
  std::vector<uint64_t> out((size_t)lines * wpl, 0);
  for (int j = 0; j < lines; ++j) {
    const long long y = vhp::window_line(o_line, j, src_lines);
    for (int k = 0; k < wpl - 2; ++k)
      out[(size_t)j * wpl + 1 + k] = vhp::window_word(y < 0 ? nullptr : src + (size_t)y * src_wpl, src_len, o_cell, len, k);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: window_driver <packed map file> <nx> <ny>   (windows \"w h ox oy\" on stdin)\n");
    return 2;
  }
  const int nx = std::atoi(argv[2]), ny = std::atoi(argv[3]);
  if (nx < 1 || ny < 1) return 2;
  const int wpr = (nx + 63) / 64 + 2, wpc = (ny + 63) / 64 + 2;
  // exactly the words of the two copies, so that a read past either one is a read past an allocation
  std::vector<uint64_t> rows((size_t)ny * wpr), cols((size_t)nx * wpc);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(rows.data(), 8, rows.size(), f) != rows.size() || std::fread(cols.data(), 8, cols.size(), f) != cols.size()) return 2;
  std::fclose(f);
  int w, h, ox, oy;
  while (std::scanf("%d %d %d %d", &w, &h, &ox, &oy) == 4) {
    if (w < 1 || h < 1) return 2;
    const std::vector<uint64_t> r = cut(rows.data(), ny, nx, oy, ox, h, w);
    const std::vector<uint64_t> c = cut(cols.data(), nx, ny, ox, oy, w, h);
    std::fwrite(r.data(), 8, r.size(), stdout);
    std::fwrite(c.data(), 8, c.size(), stdout);
  }
  return 0;
}
