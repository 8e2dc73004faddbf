// vhp_raycast_launch.h -- what vhp_capi.hip sees of the ray-cast translation unit (vhp_raycast.hip): two launches on a stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vhp_raycast.hpp"

namespace vhp {

// A batch of ray-cast fields: field s (nx * ny elements of `dtype`, a vhp_dtype with VHP_U8 allowed, packed at d_out + s * nx * ny) is
// filled with ones and cast from d_src_xy[2s..2s+1] on `occ` -- with d_map_idx on map d_map_idx[s] of the n_maps maps whose words lie
// rows_stride / cols_stride apart.  A source outside the grid or a map index outside the stack sets *d_err and leaves its field alone.
struct RaycastLaunch {
  void* d_out = nullptr;
  int dtype = 0;
  const int32_t* d_src_xy = nullptr;
  int n_src = 0;
  int nx = 0, ny = 0;
  PackedOcc occ{};
  const int32_t* d_map_idx = nullptr;
  int n_maps = 1;
  long long rows_stride = 0, cols_stride = 0;
  int* d_err = nullptr;
  hipStream_t stream = nullptr;
};
hipError_t launch_raycast(const RaycastLaunch& l);  // (hipErrorInvalidValue for a dtype that is none of the three)

// d_hit_xy[2i..2i+1]: the first blocked cell of segment d_pairs_xyxy[4i..4i+3] on occ, (-1, -1) where it is clear, (-2, -2) and *d_err
// set where an end lies outside the grid
hipError_t launch_line_of_sight(const PackedOcc& occ, int nx, int ny, const int32_t* d_pairs_xyxy, int n_pairs, int32_t* d_hit_xy, int* d_err,
                                hipStream_t stream);

}  // namespace vhp
