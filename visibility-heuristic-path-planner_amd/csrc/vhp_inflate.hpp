// vhp_inflate.hpp -- obstacles grown by a robot's footprint on the packed maps (vhp_inflate_map, vhp_inflate_maps): the footprint as a
// table of half-widths and one output word of the inflated map, written once for the device and for the host compiler (no HIP types:
// tests/inflate_driver.cpp builds it with g++).  vhp_maps.hip.h holds the kernel around it, beside the other packing kernels.
//
// A footprint is a set of integer offsets (dx, dy) picked by a shape and one integer p >= 0 (include/vhp.h vhp_footprint): a disc
// dx^2 + dy^2 <= p, a square max(|dx|, |dy|) <= p, a diamond |dx| + |dy| <= p.  Cell (x, y) of the inflated map is blocked exactly when
// some (x + dx, y + dy) is blocked in the input; cells outside the grid are free, or blocked with the border flag.  Every footprint is
// convex along a line and symmetric under x <-> y and both reflections, so it is a half-width per line offset -- hw[d], the largest
// |dx| at dy = +-d -- and the same table serves the row-packed copy (lines = rows, cells along x) and the column-packed one.
//
// On the free bits (1 = free; the layout of a packed line: vhp_window.hpp) the inflated line j is
//   free'(j) = AND over |d| <= R of erode(free(j + d), hw[|d|]),   erode(line, h) = AND of the line shifted by -h .. +h.
// R <= 64, so data word k of a line depends on words k - 1, k, k + 1 only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHP_INF_HD __host__ __device__
#else
#define VHP_INF_HD
#endif

namespace vhp {

constexpr int kMaxInflate = 64;  // VHP_MAX_INFLATE: the largest reach

// The footprint as the kernels take it (by value, in their arguments): hw[d] for d = 0 .. reach, the rest 0.
struct InflateTable {
  int reach;
  int hw[kMaxInflate + 1];
};

// floor(sqrt(v)) for 0 <= v < 2^15, in integers
VHP_INF_HD inline int inflate_isqrt(int v) {
  int r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// (shape, p) -> the table; false -- and *t untouched -- for an unknown shape, p < 0 or a reach above kMaxInflate.
// shape: 0 disc (p the squared radius), 1 square, 2 diamond.
VHP_INF_HD inline bool inflate_table(int shape, int p, InflateTable* t) {
  if (shape < 0 || shape > 2 || p < 0) return false;
  // (the disc's bound first: (kMaxInflate + 1)^2 - 1 is the last p whose reach is kMaxInflate, and past it the loop above need not run)
  if (p > (shape == 0 ? (kMaxInflate + 1) * (kMaxInflate + 1) - 1 : kMaxInflate)) return false;
  const int reach = shape == 0 ? inflate_isqrt(p) : p;
  t->reach = reach;
  for (int d = 0; d <= kMaxInflate; ++d)
    t->hw[d] = d > reach ? 0 : shape == 0 ? inflate_isqrt(p - d * d) : shape == 1 ? p : p - d;
  return true;
}

// Words k - 1, k, k + 1 of a line as one string of 192 bits, bit 0 of a[0] first.
struct InflateWords {
  uint64_t a[3];
};

// v with its bits moved down by s, 0 <= s <= 128: bit i of the result is bit i + s of v, and whatever comes in at the top is never
// looked at (below).  Whole words move as words, so that no shift count reaches 64.
VHP_INF_HD inline InflateWords inflate_down(InflateWords v, int s) {
  if (s >= 128) { v.a[0] = v.a[2]; s -= 128; }
  else if (s >= 64) { v.a[0] = v.a[1]; v.a[1] = v.a[2]; s -= 64; }
  if (s != 0) {
    v.a[0] = (v.a[0] >> s) | (v.a[1] << (64 - s));
    v.a[1] = (v.a[1] >> s) | (v.a[2] << (64 - s));
    v.a[2] >>= s;
  }
  return v;
}

// The middle word of erode(v, h), 0 <= h <= 64: bit i is the AND of bits 64 + i - h .. 64 + i + h of v.  With A_m(i) the AND of the
// m bits from i on, A_2w(i) = A_w(i) & A_w(i + w) doubles the width, one more AND at the distance m - w reaches m = 2h + 1 from the
// largest power of two w <= m, and the answer is A_m at 64 - h .. 127 - h.  A window that ends at or below bit 191 is built from
// windows inside it, so the bits that inflate_down brings in past 191 reach no bit that is read.
VHP_INF_HD inline uint64_t inflate_erode_mid(InflateWords v, int h) {
  const int m = 2 * h + 1;
  int w = 1;
  for (; 2 * w <= m; w *= 2) {
    const InflateWords s = inflate_down(v, w);
    v.a[0] &= s.a[0]; v.a[1] &= s.a[1]; v.a[2] &= s.a[2];
  }
  if (m != w) {
    const InflateWords s = inflate_down(v, m - w);
    v.a[0] &= s.a[0]; v.a[1] &= s.a[1]; v.a[2] &= s.a[2];
  }
  return inflate_down(v, 64 - h).a[0];
}

// Data word q of a packed line of `cells` cells the way the inflation reads it: the cells outside the line -- the words before and
// after it, the bits past its end, all stored as 0 -- are free unless `border` is set.  q is -1 .. (cells + 63) / 64; only the
// line's own data words are loaded.
VHP_INF_HD inline uint64_t inflate_load(const uint64_t* line, int cells, int q, bool border) {
  const int words = (cells + 63) / 64;
  if (q < 0 || q >= words) return border ? 0 : ~(uint64_t)0;
  const uint64_t v = line[1 + q];
  const int left = cells - 64 * q;  // cells of the line from bit 0 of this word on (>= 1)
  return left < 64 && !border ? v | ~(((uint64_t)1 << left) - 1) : v;
}

// Data word k (0 .. (cells + 63) / 64 - 1; stored at index 1 + k) of line j of the inflated map, from a packed copy at `base`: `lines`
// lines of `cells` cells, `stride` words apart.  A line outside the grid is all free, or with `border` all blocked.  The bits past
// the line's end come out 0, as every reader of the packed maps expects.
VHP_INF_HD inline uint64_t inflate_word(const uint64_t* base, long long stride, int lines, int cells, const InflateTable& t, bool border, int j, int k) {
  uint64_t out = ~(uint64_t)0;
  for (int d = -t.reach; d <= t.reach; ++d) {
    const int jj = j + d;
    if (jj < 0 || jj >= lines) {
      if (border) return 0;
      continue;
    }
    const uint64_t* line = base + (long long)jj * stride;
    InflateWords v;
    v.a[0] = inflate_load(line, cells, k - 1, border);
    v.a[1] = inflate_load(line, cells, k, border);
    v.a[2] = inflate_load(line, cells, k + 1, border);
    out &= inflate_erode_mid(v, t.hw[d < 0 ? -d : d]);
  }
  const int left = cells - 64 * k;
  return left < 64 ? out & (((uint64_t)1 << left) - 1) : out;
}

}  // namespace vhp
