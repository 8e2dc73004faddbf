// vhp_raycast.hip -- the ray-cast translation unit: the kernels of vhp_raycast.hip.h in their three element types behind the two
// launches of vhp_raycast_launch.h.
#include "vhp.h"

#include "vhp_raycast.hip.h"
#include "vhp_raycast_launch.h"

namespace vhp {

namespace {
template <typename OutT>
hipError_t launch_as(const RaycastLaunch& l) {
  RaycastArgs<OutT> a;
  a.out = static_cast<OutT*>(l.d_out);
  a.src_xy = l.d_src_xy;
  a.n_src = l.n_src;
  a.nx = l.nx;
  a.ny = l.ny;
  a.occ = l.occ;
  a.map_idx = l.d_map_idx;
  a.n_maps = l.n_maps;
  a.rows_stride = l.rows_stride;
  a.cols_stride = l.cols_stride;
  a.err = l.d_err;
  return launch_raycast_t(a, l.stream);
}
}  // namespace

hipError_t launch_raycast(const RaycastLaunch& l) {
  switch (l.dtype) {
    case VHP_F64: return launch_as<double>(l);
    case VHP_F32: return launch_as<float>(l);
    case VHP_U8: return launch_as<uint8_t>(l);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_line_of_sight(const PackedOcc& occ, int nx, int ny, const int32_t* d_pairs_xyxy, int n_pairs, int32_t* d_hit_xy, int* d_err,
                                hipStream_t stream) {
  if (n_pairs == 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((long long)n_pairs + kRaycastBlock - 1) / kRaycastBlock);
  hipLaunchKernelGGL(vhp_line_of_sight_kernel, dim3(blocks), dim3(kRaycastBlock), 0, stream, occ, nx, ny, d_pairs_xyxy, n_pairs, d_hit_xy, d_err);
  return hipGetLastError();
}

}  // namespace vhp
