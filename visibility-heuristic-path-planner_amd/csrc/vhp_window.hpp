// vhp_window.hpp -- a window of the packed map as packed words (vhp_set_maps_windows): the cut of one output word, written once for the
// device and for the host compiler (no HIP types: tests/window_driver.cpp builds it with g++).  vhp_maps.hip.h holds the kernels
// around it, beside the other packing kernels.
//
// A packed line (DevMap::rows: one row, packed along x; DevMap::cols: one column, packed along y) of n cells is (n + 63) / 64 + 2
// words: bit c & 63 of word 1 + (c >> 6) is cell c (1 = free), word 0 and the last word are zero pads, and the bits past n in the last
// data word are 0.  A window line of w cells that starts at cell o of such a line -- any int32 o: the window may hang over either end
// or miss the line altogether -- is the same layout for w cells, cell i of it being cell o + i of the source where that exists and
// blocked (0) where it does not: a bit-unaligned copy of words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHP_WIN_HD __host__ __device__
#else
#define VHP_WIN_HD
#endif

namespace vhp {

// Data word k (0 .. (w + 63) / 64 - 1; stored at index 1 + k) of the window line of w cells that starts at cell o of `line`, a packed
// line of n cells -- or null: a line outside the grid, all blocked.  o + 64 k is formed in 64 bits, so every int32 o is defined.
VHP_WIN_HD inline uint64_t window_word(const uint64_t* line, int n, int o, int w, int k) {
  if (!line) return 0;
  const long long first = (long long)o + 64ll * k;       // the source cell of bit 0
  const long long q = first >= 0 ? first / 64 : -((63 - first) / 64);  // floor(first / 64): the data word it lies in ...
  const int s = (int)(first - q * 64);                   // ... and its bit there, 0 .. 63 (the floor modulus)
  const long long words = ((long long)n + 63) / 64;      // data words of the source line; one outside them reads as 0
  const uint64_t lo = q >= 0 && q < words ? line[1 + q] : 0;
  uint64_t v = lo;
  if (s != 0) {                                          // (s == 0 would shift hi by 64)
    const uint64_t hi = q + 1 >= 0 && q + 1 < words ? line[1 + q + 1] : 0;
    v = (lo >> s) | (hi << (64 - s));
  }
  const int left = w - 64 * k;                           // cells the window still has from bit 0 on (>= 1)
  return left < 64 ? v & (((uint64_t)1 << left) - 1) : v;
}

// The source line of window line j for a window whose first line is line o of m lines: its index, or -1 where it lies outside 0 .. m - 1.
VHP_WIN_HD inline long long window_line(int o, int j, int m) {
  const long long y = (long long)o + j;
  return y >= 0 && y < m ? y : -1;
}

}  // namespace vhp
