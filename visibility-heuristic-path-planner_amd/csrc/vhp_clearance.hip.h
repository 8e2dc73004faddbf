// vhp_clearance.hip.h -- the kernel of vhp_map_clearance / vhp_maps_clearance around the cell functions of vhp_clearance.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "vhp_clearance.hpp"

namespace vhp {

// Rows of a workgroup's tile (its columns are the 64 cells of one data word).  With the reach R the workgroup stages TY + 2R lines of
// g and writes TY: at R = 64 that is 3 lines staged per line written with TY = 64, 2 with 128, and 5 with 32.  64 keeps the staged
// bytes at 12 KB -- no limit on the 8 workgroups of 256 threads a CU holds -- and leaves a 1000^2 map 256 tiles, one per CU, where
// 128 rows would leave half the CUs without one; at the reaches of real robots (R <= 8) the halo is a quarter of the tile or less.
constexpr int kClearanceTileRows = 64;

// The clearance field of n_maps maps from their row-packed copies: map i's ny rows of nx cells, wpr words each, at rows + i * ny * wpr,
// to out + i * nx * ny, uint16, one element per cell.  blockIdx.x is a tile -- data word `blockIdx.x % words` of kClearanceTileRows
// rows --, blockIdx.y picks the map and steps through more maps than a grid dimension holds.  A wavefront takes a row at a time, its
// lanes the 64 cells of the word: the three words of a row are uniform loads, g goes to LDS as one byte per cell (64 consecutive bytes
// a wavefront, read back the same way: no two lanes of a group on one bank with different dwords), and after the one barrier each
// thread scans the rows above and below its cells (clearance_combine) and stores 2 bytes, 128 contiguous bytes a wavefront.  No
// scratch in global memory, every element of `out` written once, offsets into it 64-bit.
__global__ void __launch_bounds__(256) vhp_clearance_stack(const uint64_t* __restrict__ rows, uint16_t* __restrict__ out, int n_maps, int nx, int ny, int wpr,
                                                           int shape, int p_max, int reach, int border) {
  __shared__ uint8_t g[(kClearanceTileRows + 2 * kMaxInflate) * 64];
  const int words = wpr - 2;
  const int q = blockIdx.x % words, y0 = (blockIdx.x / words) * kClearanceTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = 64 * q + lane;
  const int staged = kClearanceTileRows + 2 * reach;  // lines y0 - reach .. y0 + TY - 1 + reach
  for (int i = blockIdx.y; i < n_maps; i += gridDim.y) {
    const uint64_t* base = rows + (size_t)i * ny * wpr;
    if (i != (int)blockIdx.y) __syncthreads();  // (the scan of the map before still reads g)
    for (int r = wave; r < staged; r += 4) g[r * 64 + lane] = (uint8_t)clearance_line_g(base, wpr, ny, nx, border != 0, reach, x, y0 - reach + r);
    __syncthreads();
    if (x < nx) {
      uint16_t* o = out + (size_t)i * nx * ny + x;
      for (int r = wave; r < kClearanceTileRows && y0 + r < ny; r += 4)
        o[(size_t)(y0 + r) * nx] = (uint16_t)clearance_combine(shape, p_max, reach, [&](int k) { return (int)g[(reach + r + k) * 64 + lane]; });
    }
  }
}

}  // namespace vhp
