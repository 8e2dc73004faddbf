// vhp_batch_launch.h -- host-side interface of the persistent batch kernels: the pool sweep (vhp_pool.hip) and the latency
// sweep (vhp_lat.hip), used by vhp_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "vhp_devbuf.hip.h"
#include "vhp_launch_plan.hpp"
#include "vhp_stamps.hpp"

namespace vhp {

struct PlannerDev;  // (vhp_planner_dev.hip.h)

// The packed copies of n maps of one size (vhp_set_map: n = 1; vhp_set_maps: a stack, map k's words k strides after map 0's).
struct PackedMaps {
  int n = 0, nx = 0, ny = 0, wpr = 0, wpc = 0;
  DevBuf<uint64_t> rows;      // packed along x: map k's words at rows + k * ny * wpr
  DevBuf<uint64_t> cols;      // packed along y: map k's at cols + k * nx * wpc
  DevBuf<double> recip;       // one reciprocal table for max(nx, ny)
  DevBuf<uint64_t> dmap;      // packed along both diagonals (lat_pack_diag_maps / lat_pack_diag_stack): what the latency sweep reads,
                              // map k's lat_diag_map_bytes further; null where the latency sweep does not take the grid (or, for a
                              // stack, until the first planner batch on it builds them)
};

// What a latency-sweep launch from a planner's loop adds to a plain batch sweep (every member unset: a plain one).
struct LatLaunch {
  const int* src_index = nullptr;  // sweep source number *src_index of d_src (n_src = 1) ...
  const int* skip = nullptr;       // ... and nothing at all if *skip is set
  const int* pivot_rec = nullptr;  // ... or, instead of both: the 16-byte record {done, nb, x, y} of the planner's loop (LatArgs::pivot_rec)
  const int* slot_base = nullptr;  // the speculative and the batch planner's launches (LatArgs::slot_base, run_if)
  const int* run_if = nullptr;
  bool dark_unwritten = false;     // dead strips store nothing: the field holds +0.0 wherever the launch does not write
  const PlannerDev* planner_dev = nullptr;  // the launch is a whole planner iteration (launch_lat)
  // fp64, on a stack of maps (BatchArgs::n_maps of them, rows / cols / dmap those of map 0): field s is swept on map
  // map_idx[*slot_base + s] (vhp_lat.hip vhp_lat_maps_sweep) -- or null: one map
  const int32_t* map_idx = nullptr;
};

struct BatchArgs {
  const uint64_t* rows;   // packed maps and reciprocal table of the context (set_maps below)
  const uint64_t* cols;
  const double* recip;
  const uint64_t* dmap = nullptr;  // the occupancy packed along diagonals (lat_pack_diag_maps): what the latency sweep reads
  int wpr, wpc, nx, ny;
  const int32_t* d_src;   // n_src (x, y) pairs, device
  int n_src;
  void* d_out;            // n_src fields
  int dtype;              // VHP_F64 / VHP_F32
  long long field_stride; // elements
  int* d_err;             // device flag: a source outside the grid
  int* d_queue;           // the launch's scratch (pool_scratch_bytes / lat_scratch_bytes)
  int n_cus;              // compute units of the device (the persistent grid is sized to what the chip holds at once)
  int lat_workgroups = 0; // latency sweep: workgroups per octant asked for (0: by the grid's size, lat_halves)
  int* d_lat_order = nullptr;  // latency sweep: room for the launch order of its units (lat_order_bytes; vhp_lat_order), or null: none
  hipStream_t stream;
  // called with (kernel, bytes) before a launch that needs more than the default dynamic LDS: the per-device
  // bookkeeping lives with the context
  std::function<hipError_t(const void*, size_t)> raise_lds;
  // optional per-launch timing events, recorded around the launch's kernels (a timed launch that has no slot for its timestamps)
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  // ... or the launch's slot for the timestamps its own kernels write, tagged pool_epoch (vhp_stamps.hpp; pool_stamp_counts /
  // lat_stamp_counts entries of it: vhp_launch_plan.hpp); null: the kernels write none.  Plain launches only: a planner's loop passes none.
  stamps::Entry* d_stamps = nullptr;
  PoolOpts pool;          // pool sweep: the vhp_set_option keys of its launch plan (vhp_launch_plan.hpp plan_pool)
  LatLaunch lat;          // latency sweep: the launch of a planner's loop
  unsigned long long pool_epoch = 0;  // pool sweep: the tag of this launch's boundary-line entries: never 0, never reused on this scratch
  int n_maps = 0;         // maps behind rows / cols / dmap (PackedMaps::n)
};

inline void set_maps(BatchArgs& a, const PackedMaps& m) {
  a.rows = m.rows.get(); a.cols = m.cols.get(); a.recip = m.recip.get(); a.dmap = m.dmap.get();
  a.wpr = m.wpr; a.wpc = m.wpc; a.nx = m.nx; a.ny = m.ny;
  a.n_maps = m.n;
}
// ... and as the two kernels take them (map 0 of a stack)
inline geom::Map geom_map(const BatchArgs& a) { return {a.rows, a.cols, a.recip, a.wpr, a.wpc, a.nx, a.ny}; }

// The pool sweep (vhp_pool.hip): d_queue is scratch of pool_scratch_bytes (pull counter, unit order, the
// diagonal lines of the y-major units, the boundary lines of the strips) that is ZERO when it is first used and is
// written by nothing else; pool_epoch differs from launch to launch.  (pool_supported, lat_supported: defined in vhp_launch_plan.hpp)
bool pool_supported(int nx, int ny);
hipError_t launch_pool(const BatchArgs& a);
size_t pool_scratch_bytes(int n_src, int nx, int ny);

// The latency sweep (vhp_lat.hip): one workgroup per octant, for launches of a few sources.  d_queue is scratch of
// lat_scratch_bytes with the pool sweep's rules (zero when first used, written by nothing but these two kernels; the two
// share the epoch counter, so either may follow the other on one allocation).
bool lat_supported(int nx, int ny);
// With a.lat.planner_dev (d), a planner iteration as one launch: the latency sweep of the pivot named by a.lat.pivot_rec (fp64, into
// a.d_out) and, in the same grid, the epilogue over d (union, labels, heuristic, next pivot: vhp_planner_dev.hip.h).  d.ticket[1] counts
// the sweep's workgroups.
hipError_t launch_lat(const BatchArgs& a);
size_t lat_scratch_bytes(int n_src, int nx, int ny);
size_t lat_order_bytes();
// The latency sweep's lanes run along diagonals of the grid: it reads the occupancy packed along them (vhp_band.hpp DiagMaps),
// built once per map from the byte map: lat_diag_map_bytes of device memory, zero-filled and packed by lat_pack_diag_maps.
size_t lat_diag_map_bytes(int nx, int ny);
hipError_t lat_pack_diag_maps(const uint8_t* d_occ, int nx, int ny, uint64_t* d_dmap, hipStream_t stream);
// ... and for a stack of n_maps maps from their row-packed words (map k's at d_rows + k * ny * wpr): map k's diagonal maps at
// d_dmap + k * lat_diag_map_bytes(nx, ny) / 8, every word written
hipError_t lat_pack_diag_stack(const uint64_t* d_rows, int n_maps, int nx, int ny, int wpr, uint64_t* d_dmap, hipStream_t stream);

}  // namespace vhp
