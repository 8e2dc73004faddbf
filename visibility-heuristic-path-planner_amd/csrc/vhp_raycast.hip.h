// vhp_raycast.hip.h -- ray-cast visibility for batches of sources and line-of-sight tests of segments, on the packed maps
// (vhp_raycast.hpp: the ray walk and the launch plan; vhp_raycast.hip: the translation unit; vhp_capi.hip: vhp_raycast_[maps_]batch[_device],
// vhp_line_of_sight[_device], through vhp_raycast_launch.h).
//   vhp_raycast_fill    every field of a source that is cast set to 1 (the reference's reset(), solver.cpp:45)
//   vhp_raycast_fields  one thread per (source, target): the ray walked, and where it is blocked the blocked cell and the target zeroed
//   vhp_line_of_sight_kernel  one thread per segment: the first blocked cell or (-1, -1)
// After the fill every store is a zero: the result does not depend on the order of the rays, two threads that store to one cell store
// the same value, and no thread stores its own 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vhp_raycast.hpp"

namespace vhp {

// What both field kernels take: the fields, the sources, the map or the stack (map_idx null: the single map `occ`).
template <typename OutT>
struct RaycastArgs {
  OutT* out;               // field s at out + s * cells
  const int32_t* src_xy;
  int n_src;
  int nx, ny;
  PackedOcc occ;           // map 0
  const int32_t* map_idx;  // a stack: source s is cast on map map_idx[s] of n_maps, whose words lie map_idx[s] times the strides further
  int n_maps;
  long long rows_stride, cols_stride;
  int* err;                // set where a source is not cast (vhp_sync)
};

template <typename OutT>
__global__ void __launch_bounds__(kRaycastBlock) vhp_raycast_fill(RaycastArgs<OutT> a) {
  constexpr int kPer = 16 / (int)sizeof(OutT);  // elements of a 16-byte store
  typedef OutT Vec __attribute__((ext_vector_type(kPer)));
  Vec ones;
  for (int j = 0; j < kPer; ++j) ones[j] = OutT(1);
  const long long cells = (long long)a.nx * a.ny;
  raycast_for_sources(blockIdx.y, gridDim.y, a.n_src, [&](int s) {
    if (!raycast_source_ok(a.src_xy, a.map_idx, s, a.nx, a.ny, a.n_maps)) return;  // (a field that is not cast is not written)
    OutT* const f = a.out + (long long)s * cells;
    // the elements before the first 16-byte boundary, whole 16-byte pieces, the elements behind the last
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(f) & 15)) & 15) / (long long)sizeof(OutT);
    if (head > cells) head = cells;
    const long long n_vec = (cells - head) / kPer, tail = cells - head - n_vec * kPer;
    Vec* const fv = reinterpret_cast<Vec*>(f + head);
    for (long long i = (long long)blockIdx.x * kRaycastBlock + threadIdx.x; i < n_vec; i += (long long)gridDim.x * kRaycastBlock) fv[i] = ones;
    if (blockIdx.x == 0) {
      if ((long long)threadIdx.x < head) f[threadIdx.x] = OutT(1);
      if ((long long)threadIdx.x < tail) f[head + n_vec * kPer + threadIdx.x] = OutT(1);
    }
  });
}

template <typename OutT>
__global__ void __launch_bounds__(kRaycastBlock) vhp_raycast_fields(RaycastArgs<OutT> a) {
  const long long cells = (long long)a.nx * a.ny;
  const long long k = (long long)blockIdx.x * kRaycastBlock + threadIdx.x;
  const int x1 = (int)(k % a.nx), y1 = (int)(k / a.nx);
  raycast_for_sources(blockIdx.y, gridDim.y, a.n_src, [&](int s) {
    if (!raycast_source_ok(a.src_xy, a.map_idx, s, a.nx, a.ny, a.n_maps)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, 1);
      return;
    }
    if (k >= cells) return;
    PackedOcc occ = a.occ;
    if (a.map_idx) {
      occ.rows += a.map_idx[s] * a.rows_stride;
      occ.cols += a.map_idx[s] * a.cols_stride;
    }
    int hx, hy;
    if (ray_walk(occ, a.src_xy[2 * (size_t)s], a.src_xy[2 * (size_t)s + 1], x1, y1, &hx, &hy)) {
      OutT* const f = a.out + (long long)s * cells;
      f[(long long)hy * a.nx + hx] = OutT(0);
      f[k] = OutT(0);
    }
  });
}

// pairs_xyxy: (x0, y0, x1, y1) per segment; hit_xy: the first blocked cell, (-1, -1) where the segment is clear, (-2, -2) and *err set
// where an end lies outside the grid
__global__ void __launch_bounds__(kRaycastBlock) vhp_line_of_sight_kernel(PackedOcc occ, int nx, int ny, const int32_t* __restrict__ pairs_xyxy,
                                                                          int n_pairs, int32_t* __restrict__ hit_xy, int* err) {
  const long long i = (long long)blockIdx.x * kRaycastBlock + threadIdx.x;
  if (i >= n_pairs) return;
  const int x0 = pairs_xyxy[4 * i], y0 = pairs_xyxy[4 * i + 1], x1 = pairs_xyxy[4 * i + 2], y1 = pairs_xyxy[4 * i + 3];
  int hx = -1, hy = -1;
  if (x0 < 0 || y0 < 0 || x0 >= nx || y0 >= ny || x1 < 0 || y1 < 0 || x1 >= nx || y1 >= ny) {
    hx = hy = -2;
    atomicOr(err, 1);
  } else if (!ray_walk(occ, x0, y0, x1, y1, &hx, &hy)) {
    hx = hy = -1;
  }
  hit_xy[2 * i] = hx;
  hit_xy[2 * i + 1] = hy;
}

// fill + cast on `stream`; nothing where the batch is empty
template <typename OutT>
inline hipError_t launch_raycast_t(const RaycastArgs<OutT>& a, hipStream_t stream) {
  const RaycastPlan p = plan_raycast((long long)a.nx * a.ny, a.n_src);
  if (p.grid_y == 0) return hipSuccess;
  // (the fill's threads store 16 bytes each: a sixteenth of the tiles in x covers a field of bytes once, the loop does the rest)
  const unsigned fill_x = (p.tiles + 15) / 16;
  hipLaunchKernelGGL(vhp_raycast_fill<OutT>, dim3(fill_x, p.grid_y), dim3(p.block), 0, stream, a);
  hipLaunchKernelGGL(vhp_raycast_fields<OutT>, dim3(p.tiles, p.grid_y), dim3(p.block), 0, stream, a);
  return hipGetLastError();
}

}  // namespace vhp
