// vhp_paths.hpp -- reconstructPath() (reference src/visibilityBasedSolver.cpp:1183-1213) over a planner result that stays in device
// memory: the two bodies of the device route, written once for the device and for the host compiler (no HIP types: tests/paths_driver.cpp
// builds them with g++ and feeds them tables).  The contract is vhp_reconstruct_path's (vhp_capi.hip), check for check and in its order:
//   t = label[end]; until the label repeats: note the point; a label above n_pivots -> VHP_ERR_ARG; more than n_pivots + 2 points noted ->
//   VHP_ERR_ARG; the pivot outside the grid -> VHP_ERR_ARG; t = label[pivot].  Then the last point, the path turned start-first, the
//   length summed from the start's end, one segment after the other (fp64 addition is not associative: no tree, no partial sums).
// Two steps (vhp_paths.hip.h launches them over all queries of a solve):
//   paths_parent_entry : parent[k] = label[pivot k] for k = 0 .. n_pivots -- the only reads of the nx * ny label field, one independent
//                        gather per thread; a pivot outside the grid gives kPathsPivotOob, so that the walk never indexes the field.
//   paths_walk         : one thread per query; every hop is a load from that small table instead of a trip into the label field.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHP_PATHS_HD __host__ __device__
#else
#define VHP_PATHS_HD
#endif

namespace vhp {

// the status codes of include/vhp.h the walk can return (this header includes no other)
constexpr int kPathsOk = 0, kPathsErrArg = 1, kPathsErrTooLarge = 102;
// parent[] of a pivot that lies outside the grid.  Like an unlabelled cell's 0xFFFFFFFF it is above every n_pivots (<= 2^24 + 8), and both
// end the host walk with VHP_ERR_ARG.
constexpr uint32_t kPathsPivotOob = 0xfffffffeu;

// eval_d, visibilityBasedSolver.h:112-115: first product in double, second in int; the square root correctly rounded
VHP_PATHS_HD inline double paths_eval_d(int ax, int ay, int bx, int by) {
  const int dx = ax - bx, dy = ay - by;
  return __builtin_sqrt((double)dx * dx + (double)(dy * dy));
}

// Step 1, entry k of a query's parent table: the label of pivot k's cell (label: the query's nx * ny labels, 0xFFFFFFFF = unlabelled).
VHP_PATHS_HD inline uint32_t paths_parent_entry(const uint32_t* label, const int32_t* pivots_xy, uint32_t k, int nx, int ny) {
  const int x = pivots_xy[2 * (size_t)k], y = pivots_xy[2 * (size_t)k + 1];
  if (x < 0 || y < 0 || x >= nx || y >= ny) return kPathsPivotOob;
  return label[(size_t)x + (size_t)y * nx];
}

// Step 2, one query.  end_label: label[end] (end inside the grid: the solve validated it); parent: n_pivots + 1 entries of step 1;
// pivots_xy: entries 0 .. n_pivots; rev: room for 2 * (n_pivots + 3) ints, the points end-first (the host's `rev`).
// path_xy: cap points of room or null (counts and length only, cap ignored, never kPathsErrTooLarge).
// Returns the status; *n_path and *length are the host's on kPathsOk and kPathsErrTooLarge, and 0 on kPathsErrArg (where the host
// leaves its outputs alone).  Nothing is written to path_xy unless the status is kPathsOk.
VHP_PATHS_HD inline int paths_walk(uint32_t end_label, const uint32_t* parent, const int32_t* pivots_xy, uint32_t n_pivots, int end_x,
                                   int end_y, int32_t* rev, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length) {
  *n_path = 0;
  *length = 0.0;
  int x = end_x, y = end_y;
  uint32_t n = 0;
  // (64 bits: no label equals the initial t_old, as on the host, where it is UINT64_MAX against labels of at most 1e15)
  uint64_t t = end_label, t_old = ~(uint64_t)0;
  while (t != t_old) {
    rev[2 * (size_t)n] = x;
    rev[2 * (size_t)n + 1] = y;
    ++n;
    t_old = t;
    if (t > n_pivots) return kPathsErrArg;        // an unlabelled cell, a pivot outside the grid one hop ago, or a label outside the list
    if (n > n_pivots + 2) return kPathsErrArg;    // the labels form a cycle
    x = pivots_xy[2 * (size_t)t];
    y = pivots_xy[2 * (size_t)t + 1];
    const uint32_t p = parent[t];
    if (p == kPathsPivotOob) return kPathsErrArg; // (the host's range check on (x, y), made when the table was built)
    t = p;
  }
  rev[2 * (size_t)n] = x;
  rev[2 * (size_t)n + 1] = y;
  ++n;
  // start-first: point k of the path is rev[n - 1 - k]; ONE running sum in path order
  double total = 0.0;
  for (uint32_t k = n - 1; k > 0; --k)
    total += paths_eval_d(rev[2 * (size_t)k], rev[2 * (size_t)k + 1], rev[2 * (size_t)k - 2], rev[2 * (size_t)k - 1]);
  *n_path = n;
  *length = total;
  if (path_xy) {
    if (n > cap) return kPathsErrTooLarge;
    for (uint32_t k = 0; k < n; ++k) {
      path_xy[2 * (size_t)k] = rev[2 * (size_t)(n - 1 - k)];
      path_xy[2 * (size_t)k + 1] = rev[2 * (size_t)(n - 1 - k) + 1];
    }
  }
  return kPathsOk;
}

}  // namespace vhp
