// vhp_maps.hip.h -- the map layer: the kernels that write and read the packed occupancy maps (PackedMaps, vhp_batch_launch.h), and
// the host operations over them.  The operations take a PackedMaps and a stream, enqueue on that stream and return HIP's error: they
// know nothing of a context, its scratch or its error text (vhp_capi.hip: the one includer).  A single map is a stack of one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "vhp_batch_launch.h"
#include "vhp_inflate.hpp"
#include "vhp_sweep.hip.h"  // (kRecipPad: how far past max(nx, ny) the sweeps read the reciprocal table)
#include "vhp_window.hpp"

namespace vhp {

// ---------------------------------------------------------------------------
// map packing: one wavefront per 64 cells, ballot -> one word
// ---------------------------------------------------------------------------
// A stack of n_maps maps of nx x ny (map k at occ + k*nx*ny, its words at rows + k*ny*wpr / cols + k*nx*wpc):
// one launch per copy, blockIdx.y picks the map (stepping by gridDim.y past 65535 maps).
__global__ void vhp_pack_rows_stack(const uint8_t* __restrict__ occ, uint64_t* __restrict__ rows, int n_maps, int nx, int ny, int wpr) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int words = wpr - 2;
  if (wave >= words * ny) return;
  const int y = wave / words, w = wave - y * words;
  const int x = w * 64 + lane;
  for (int k = blockIdx.y; k < n_maps; k += gridDim.y) {
    const bool f = x < nx && occ[(size_t)k * nx * ny + (size_t)y * nx + x] != 0;
    const uint64_t b = __ballot(f);
    if (lane == 0) rows[(size_t)k * ny * wpr + (size_t)y * wpr + 1 + w] = b;
  }
}

__global__ void vhp_pack_cols_stack(const uint8_t* __restrict__ occ, uint64_t* __restrict__ cols, int n_maps, int nx, int ny, int wpc) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int words = wpc - 2;
  if (wave >= words * nx) return;
  const int x = wave / words, w = wave - x * words;
  const int y = w * 64 + lane;
  for (int k = blockIdx.y; k < n_maps; k += gridDim.y) {
    const bool f = y < ny && occ[(size_t)k * nx * ny + (size_t)y * nx + x] != 0;
    const uint64_t b = __ballot(f);
    if (lane == 0) cols[(size_t)k * nx * wpc + (size_t)x * wpc + 1 + w] = b;
  }
}

// A stack of n_win windows of w x h cut from the packed copies of one nx x ny map (vhp_set_maps_windows): window k starts at the map's
// cell (origin_xy[2k], origin_xy[2k+1]), any int32.  One thread per data word (vhp_window.hpp window_word), the pads left to the
// caller's memset; blockIdx.y picks the window as above.  Neighbouring threads read neighbouring words of one source line.
__global__ void vhp_cut_rows_stack(const uint64_t* __restrict__ src_rows, int nx, int ny, int src_wpr, const int32_t* __restrict__ origin_xy,
                                   uint64_t* __restrict__ rows, int n_win, int w, int h, int wpr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int words = wpr - 2;
  if (t >= words * h) return;
  const int j = t / words, k = t - j * words;
  for (int i = blockIdx.y; i < n_win; i += gridDim.y) {
    const long long y = window_line(origin_xy[2 * i + 1], j, ny);
    rows[(size_t)i * h * wpr + (size_t)j * wpr + 1 + k] = window_word(y < 0 ? nullptr : src_rows + (size_t)y * src_wpr, nx, origin_xy[2 * i], w, k);
  }
}

// ... and the column-packed copy: the same cut along y of the map's columns
__global__ void vhp_cut_cols_stack(const uint64_t* __restrict__ src_cols, int nx, int ny, int src_wpc, const int32_t* __restrict__ origin_xy,
                                   uint64_t* __restrict__ cols, int n_win, int w, int h, int wpc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int words = wpc - 2;
  if (t >= words * w) return;
  const int j = t / words, k = t - j * words;
  for (int i = blockIdx.y; i < n_win; i += gridDim.y) {
    const long long x = window_line(origin_xy[2 * i], j, nx);
    cols[(size_t)i * w * wpc + (size_t)j * wpc + 1 + k] = window_word(x < 0 ? nullptr : src_cols + (size_t)x * src_wpc, ny, origin_xy[2 * i + 1], h, k);
  }
}

// Maps first .. first + n - 1 of a stack back to one byte per cell (1 = free), from the row-packed copy (vhp_maps_occupancy): one
// thread per cell of a map, blockIdx.y picks the map as above; rows points at map `first`.
__global__ void vhp_unpack_rows_stack(const uint64_t* __restrict__ rows, uint8_t* __restrict__ occ, int n, int nx, int ny, int wpr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nx * ny) return;
  const int y = c / nx, x = c - y * nx;
  for (int k = blockIdx.y; k < n; k += gridDim.y)
    occ[(size_t)k * nx * ny + c] = (rows[(size_t)k * ny * wpr + (size_t)y * wpr + 1 + (x >> 6)] >> (x & 63)) & 1;
}

// One packed copy of n_maps maps with their obstacles grown by a footprint (vhp_inflate_map, vhp_inflate_maps): map i's `lines` lines
// of `cells` cells, wpl words each, at src + i * lines * wpl, inflated to the same place of dst -- never src itself: a word is read by
// up to 129 lines' threads.  The row-packed copy takes (lines, cells, wpl) = (ny, nx, wpr), the column-packed one (nx, ny, wpc): the
// footprints are symmetric under x <-> y (vhp_inflate.hpp), so one kernel serves both.  One thread per data word, neighbouring
// threads on neighbouring words of one line, the pads left to the caller; blockIdx.y picks the map as above.  The table is uniform
// and indexed by the uniform loop counter: it stays in the kernel arguments.
__global__ void __launch_bounds__(256) vhp_inflate_stack(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int n_maps, int lines, int cells,
                                                         int wpl, InflateTable tab, int border) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int words = wpl - 2;
  if (t >= words * lines) return;
  const int j = t / words, k = t - j * words;
  for (int i = blockIdx.y; i < n_maps; i += gridDim.y) {
    const size_t at = (size_t)i * lines * wpl;
    dst[at + (size_t)j * wpl + 1 + k] = inflate_word(src + at, wpl, lines, cells, tab, border != 0, j, k);
  }
}

}  // namespace vhp

#include "vhp_clearance.hip.h"  // the clearance field of the packed maps: a kernel of its own file

namespace vhp {

// The grid of a stack kernel: blocks of 256 threads, `threads` of them per map along x, the map along y (the kernels step through
// more maps than a grid dimension holds).
inline dim3 stack_grid(long long threads, int n) { return dim3((unsigned)((threads + 255) / 256), (unsigned)std::min(n, 65535)); }

// Map k's words in the two packed copies of m: k strides after map 0's.
inline uint64_t* map_rows(const PackedMaps& m, int k) { return m.rows.get() + (size_t)k * m.ny * m.wpr; }
inline uint64_t* map_cols(const PackedMaps& m, int k) { return m.cols.get() + (size_t)k * m.nx * m.wpc; }

// RN(1/k) for k = 1 .. max(nx, ny) + kRecipPad, and 0 for k = 0
inline std::vector<double> recip_table(int nx, int ny) {
  const int nrec = std::max(nx, ny) + 1 + kRecipPad;
  std::vector<double> recip(nrec);
  recip[0] = 0.0;
  for (int k = 1; k < nrec; ++k) {
    volatile double d = (double)k;
    recip[k] = 1.0 / d;  // correctly rounded IEEE division on the host
  }
  return recip;
}

// The packed copies of n maps of nx x ny into m, which comes in empty: allocated and zeroed, filled by fill(t) -- t: the maps with
// their sizes, seen by nobody else yet --, the reciprocal table uploaded, the stream synchronised.  m gets its sizes, and its arrays,
// only once all of it is on the device; until then, and after a failure, it stays empty, and the caller drops what else belonged to it.
template <typename Fill>
hipError_t maps_build(PackedMaps& m, int n, int nx, int ny, hipStream_t stream, Fill fill) {
  PackedMaps t;
  t.n = n; t.nx = nx; t.ny = ny; t.wpr = (nx + 63) / 64 + 2; t.wpc = (ny + 63) / 64 + 2;
  const size_t rows_bytes = (size_t)n * ny * t.wpr * 8, cols_bytes = (size_t)n * nx * t.wpc * 8;
  hipError_t e = t.rows.grow(rows_bytes);
  if (e == hipSuccess) e = t.cols.grow(cols_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(t.rows.get(), 0, rows_bytes, stream);
  if (e == hipSuccess) e = hipMemsetAsync(t.cols.get(), 0, cols_bytes, stream);
  if (e == hipSuccess) e = fill(t);
  if (e != hipSuccess) return e;
  const std::vector<double> recip = recip_table(nx, ny);
  e = t.recip.grow(recip.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(t.recip.get(), recip.data(), recip.size() * sizeof(double), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e == hipSuccess) m = std::move(t);
  return e;
}

// Both packed copies of m from its maps' bytes at d_occ (map k's nx * ny further): one launch per copy, a wavefront per data word.
inline hipError_t maps_pack(PackedMaps& m, const uint8_t* d_occ, hipStream_t stream) {
  hipLaunchKernelGGL(vhp_pack_rows_stack, stack_grid((long long)(m.wpr - 2) * m.ny * 64, m.n), dim3(256), 0, stream, d_occ, m.rows.get(), m.n, m.nx, m.ny, m.wpr);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(vhp_pack_cols_stack, stack_grid((long long)(m.wpc - 2) * m.nx * 64, m.n), dim3(256), 0, stream, d_occ, m.cols.get(), m.n, m.nx, m.ny, m.wpc);
  return hipGetLastError();
}

// Both packed copies of m as m.n windows of m.nx x m.ny of the single map s, cut from its packed copies at the (x, y) origins at
// d_origin: one launch per copy, a thread per data word.
inline hipError_t maps_cut(PackedMaps& m, const PackedMaps& s, const int32_t* d_origin, hipStream_t stream) {
  hipLaunchKernelGGL(vhp_cut_rows_stack, stack_grid((long long)(m.wpr - 2) * m.ny, m.n), dim3(256), 0, stream, s.rows.get(), s.nx, s.ny, s.wpr, d_origin,
                     m.rows.get(), m.n, m.nx, m.ny, m.wpr);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(vhp_cut_cols_stack, stack_grid((long long)(m.wpc - 2) * m.nx, m.n), dim3(256), 0, stream, s.cols.get(), s.nx, s.ny, s.wpc, d_origin,
                     m.cols.get(), m.n, m.nx, m.ny, m.wpc);
  return hipGetLastError();
}

// n maps of nx x ny from their row-packed words at `rows` (wpr a row) as bytes at d_out, and maps first .. first + n - 1 of m.
inline hipError_t maps_unpack(const uint64_t* rows, int n, int nx, int ny, int wpr, uint8_t* d_out, hipStream_t stream) {
  hipLaunchKernelGGL(vhp_unpack_rows_stack, stack_grid((long long)nx * ny, n), dim3(256), 0, stream, rows, d_out, n, nx, ny, wpr);
  return hipGetLastError();
}
inline hipError_t maps_unpack(const PackedMaps& m, int first, int n, uint8_t* d_out, hipStream_t stream) {
  return maps_unpack(map_rows(m, first), n, m.nx, m.ny, m.wpr, d_out, stream);
}

// One packed copy of n maps -- `lines` lines of `cells` cells, wpl words each, from src on -- inflated by the footprint t to dst
// (vhp_inflate_stack: one thread per data word, the pads of dst the caller's).
inline hipError_t maps_inflate_copy(const uint64_t* src, uint64_t* dst, int n, int lines, int cells, int wpl, const InflateTable& t, int border,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(vhp_inflate_stack, stack_grid((long long)(wpl - 2) * lines, n), dim3(256), 0, stream, src, dst, n, lines, cells, wpl, t, border);
  return hipGetLastError();
}

// The clearance field of maps first .. first + n - 1 of m at d_out, nx * ny elements a map: one launch (vhp_clearance_stack), a
// workgroup per tile.
inline hipError_t maps_clearance(const PackedMaps& m, int first, int n, int shape, int p_max, int reach, int border, uint16_t* d_out, hipStream_t stream) {
  const long long tiles = (long long)(m.wpr - 2) * ((m.ny + kClearanceTileRows - 1) / kClearanceTileRows);
  hipLaunchKernelGGL(vhp_clearance_stack, stack_grid(tiles * 256, n), dim3(256), 0, stream, map_rows(m, first), d_out, n, m.nx, m.ny, m.wpr, shape, p_max,
                     reach, border);
  return hipGetLastError();
}

}  // namespace vhp
