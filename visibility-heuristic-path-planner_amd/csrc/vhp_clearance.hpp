// vhp_clearance.hpp -- the clearance field of the packed maps (vhp_map_clearance, vhp_maps_clearance): for every cell the smallest
// footprint parameter p at which vhp_inflate_map(shape, p, flags) would block it, written once for the device and for the host compiler
// (no HIP types: tests/clearance_driver.cpp builds it with g++).  vhp_clearance.hip.h holds the kernel around it.
//
// With the metric m(dx, dy) of a shape -- dx^2 + dy^2 for a disc, max(|dx|, |dy|) for a square, |dx| + |dy| for a diamond: the left
// sides of the footprints' predicates (vhp_inflate.hpp) -- the clearance c(x, y) is the minimum of m(dx, dy) over every (dx, dy) for
// which cell (x + dx, y + dy) is blocked, cells outside the grid being free, or blocked with the border flag; the field holds c where
// c <= p_max and kClearanceFar elsewhere.  A blocked cell holds 0, and (c > p) is the map inflated by (shape, p) for every p <= p_max.
//
// All three metrics are min-plus separable and grow with |dx| and with |dy|:
//   c(x, y) = min over |k| <= R of m(g(x, y + k), k),   g(x, j) = the distance along line j from x to its nearest blocked cell,
// R = reach(p_max) <= 64 -- an offset with a larger |dx| or |dy| has a metric above p_max.  So g for the 64 cells of data word q of a
// line depends on words q - 1, q, q + 1 only, the 192 bits inflate_load hands the inflation, cells past the line's end included; the
// nearest zero bit on either side of a cell is one count of leading and one of trailing zeros, no loop over cells.  The footprints are
// symmetric under x <-> y, so the same functions serve the row-packed copy (lines = rows) and the column-packed one.
#pragma once
#include <stdint.h>

#include "vhp_inflate.hpp"

namespace vhp {

constexpr unsigned kClearanceFar = 0xFFFF;  // VHP_CLEARANCE_FAR: no blocked cell within p_max
constexpr int kClearanceNone = 255;         // g of a line without a blocked cell within the reach: a byte whose metric is above any p_max

VHP_INF_HD inline int clearance_clz(uint64_t v) { return __builtin_clzll(v); }  // v != 0
VHP_INF_HD inline int clearance_ctz(uint64_t v) { return __builtin_ctzll(v); }  // v != 0

// g for bit 64 + i (0 <= i < 64) of the string v of free bits (1 = free, inflate_load's words q - 1, q, q + 1): 0 on a blocked
// cell, else the distance to the nearest 0 bit among the 64 on either side, or kClearanceNone if that is none or lies beyond `reach`.
// No shift count reaches 64.
VHP_INF_HD inline int clearance_word_g(const InflateWords& v, int i, int reach) {
  const uint64_t b0 = ~v.a[0], b1 = ~v.a[1], b2 = ~v.a[2];  // 1 = blocked
  if ((b1 >> i) & 1) return 0;
  // bits 64 + i - 64 .. 64 + i - 1, the nearest at the top; bits 64 + i + 1 .. 64 + i + 64, the nearest at the bottom
  const uint64_t below = i == 0 ? b0 : (b0 >> i) | (b1 << (64 - i));
  const uint64_t above = i == 63 ? b2 : (b1 >> (i + 1)) | (b2 << (63 - i));
  int g = kClearanceNone;
  if (below != 0) g = clearance_clz(below) + 1;
  if (above != 0) {
    const int d = clearance_ctz(above) + 1;
    if (d < g) g = d;
  }
  return g <= reach ? g : kClearanceNone;
}

// The per-row function: g(x, j) on a packed copy at `base` -- `lines` lines of `cells` cells, `stride` words apart -- for
// 0 <= x < 64 * ((cells + 63) / 64) and any j.  A line outside the grid is all blocked with `border` (0) and has nothing without it.
VHP_INF_HD inline int clearance_line_g(const uint64_t* base, long long stride, int lines, int cells, bool border, int reach, int x, int j) {
  if (j < 0 || j >= lines) return border ? 0 : kClearanceNone;
  const uint64_t* line = base + (long long)j * stride;
  const int q = x >> 6;
  InflateWords v;
  v.a[0] = inflate_load(line, cells, q - 1, border);
  v.a[1] = inflate_load(line, cells, q, border);
  v.a[2] = inflate_load(line, cells, q + 1, border);
  return clearance_word_g(v, x & 63, reach);
}

// The reach of a valid (shape, p_max), as inflate_table has it
VHP_INF_HD inline int clearance_reach(int shape, int p_max) { return shape == 0 ? inflate_isqrt(p_max) : p_max; }

// m(g, k) for k >= 0 and g >= 0; with g = kClearanceNone the result is above any valid p_max (255^2, 255, 255 against 4224, 64, 64).
VHP_INF_HD inline int clearance_metric(int shape, int g, int k) { return shape == 0 ? g * g + k * k : shape == 1 ? (g > k ? g : k) : g + k; }

// The combining function: the output for one cell from g_at(k) = g(x, y + k), |k| <= reach.  The lines are taken in the order
// k = 0, +-1, +-2, ... and the scan stops at the first k whose own metric m(0, k) is no better than the best so far: every m(g, k')
// with k' >= k is at least that.  `best` starts at p_max + 1, so a cell with nothing within p_max stops at the reach and is far.
template <typename G>
VHP_INF_HD inline unsigned clearance_combine(int shape, int p_max, int reach, G g_at) {
  int best = p_max + 1;
  for (int k = 0; k <= reach && clearance_metric(shape, 0, k) < best; ++k) {
    const int up = clearance_metric(shape, g_at(k), k);
    if (up < best) best = up;
    if (k != 0) {
      const int down = clearance_metric(shape, g_at(-k), k);
      if (down < best) best = down;
    }
  }
  return best <= p_max ? (unsigned)best : kClearanceFar;
}

// The clearance of cell x of line y of a packed copy (x along the lines), as the kernel computes it: the same two functions, g read
// from the packed words here and from its staged bytes there.  (shape, p_max) must be valid (inflate_table).
VHP_INF_HD inline unsigned clearance_cell(const uint64_t* base, long long stride, int lines, int cells, int shape, int p_max, bool border, int x, int y) {
  const int reach = clearance_reach(shape, p_max);
  return clearance_combine(shape, p_max, reach, [&](int k) { return clearance_line_g(base, stride, lines, cells, border, reach, x, y + k); });
}

}  // namespace vhp
