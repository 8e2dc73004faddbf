// vhp_pool_scratch.hpp -- how the pool sweep's launcher (vhp_pool.hip) sizes the scratch of a launch.  Host code without a HIP
// header, so that tests/pool_scratch_driver.cpp can hold the sizes against what UnitGeo (vhp_pool.hpp) asks for, on the CPU.
#pragma once
#include <cstddef>

#include "vhp_pool.hpp"

namespace vhp {
namespace {
constexpr int kQueueInts = 16;  // the pull counter (and padding) ahead of the order array

// scratch of a launch: [pull counter, recs[4 n_units], order[n_units], line_base[n_units]] [diagonal lines] [boundary lines]
int diag_stride_of(int nx, int ny) { return ((nx < ny ? nx : ny) + 64 + 15) & ~15; }
size_t head_bytes(int n_src) { return (((size_t)(kQueueInts + 6 * pool::kUnits * (size_t)n_src) * sizeof(int)) + 255) & ~(size_t)255; }
size_t diag_bytes(int n_src, int nx, int ny) { return (((size_t)n_src * 4 * (size_t)diag_stride_of(nx, ny) * sizeof(double)) + 255) & ~(size_t)255; }
// 64-entry blocks of boundary lines a source can need, an upper bound: over its four quadrants ni * nj sums to nx * ny;
// an x-major unit takes at most (min(ni,nj)/64) * (ni/64 + 2) blocks, a y-major one (ni/128 + 1) * (nj/64 + 2)
long long line_blocks_per_source(int nx, int ny) { return (3LL * nx * ny) / 8192 + (nx + ny) / 4 + 64; }
}  // namespace
}  // namespace vhp
