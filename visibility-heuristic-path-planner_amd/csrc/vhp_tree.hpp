// vhp_tree.hpp -- the whole tree a planner solve leaves in device memory, read from any cell: the path length to every cell (a
// cost-to-come field per query) and the path to any goal.  Every cell some pivot lit carries that pivot's label, every pivot's own cell
// the label of the pivot that lit it; reconstructPath() (reference src/visibilityBasedSolver.cpp:1183-1213) walks that tree from one
// cell.  The contract is vhp_reconstruct_path's (vhp_capi.hip) from ANY cell (x, y): status, point count, points and the fp64 bits of
// the length.  The bodies are written once, for the device and for the host compiler (no HIP types: tests/tree_driver.cpp builds them
// with g++ and feeds them tables).
//
// What the host's walk from a cell with label L does, restated per pivot.  With parent[t] = label[pivot t] (vhp_paths.hpp
// paths_parent_entry; kPathsPivotOob for a pivot outside the grid) the walk visits L, parent[L], parent[parent[L]], ... and stops at
// the first node that is its own parent.  It fails with VHP_ERR_ARG on a node above n_pivots (an unlabelled cell's 0xFFFFFFFF and
// kPathsPivotOob are both above), on a pivot outside the grid, and after n_pivots + 2 points (a cycle that is not a self-loop; a walk
// that ends visits at most n_pivots + 1 distinct nodes, so the bound never cuts a good one).  So per pivot t:
//   depth[t] = hops from t to the self-loop it reaches, kTreeInvalid if the walk from t fails     (tree_depth_entry, a bounded walk)
//   cum[t]   = cum[parent[t]] + eval_d(pivot[parent[t]], pivot[t]), cum[root] = 0                  (tree_cum_entry, level by level)
// and per cell (tree_cell): valid iff L <= n_pivots and depth[L] != kTreeInvalid; n_path = depth[L] + 2 (the cell, pivot L, its
// ancestors); length = cum[L] + eval_d(pivot[L], cell).  That is the host's association order -- ONE running sum from the start's end
// of the path, 0.0 + d1 + d2 + ... -- so the bits agree; any tree-shaped or reordered sum would not.
// No table, consistent or not, is read out of bounds: every index is checked against n_pivots before it is used, and every walk is
// bounded by n_pivots + 2 hops (cycles, roots other than 0 and parent[t] > t included).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vhp_paths.hpp"

namespace vhp {

// the fourth status code of include/vhp.h these bodies return (beside kPathsOk, kPathsErrArg, kPathsErrTooLarge)
constexpr int kTreeErrEndOob = 11;
// depth[] of a pivot the host's walk fails from (real depths are at most n_pivots <= 2^24 + 8)
constexpr uint32_t kTreeInvalid = 0xffffffffu;

// Entry t of a query's depth table (t <= n_pivots; parent: n_pivots + 1 entries).  At most n_pivots + 2 loads.
VHP_PATHS_HD inline uint32_t tree_depth_entry(const uint32_t* parent, uint32_t n_pivots, uint32_t t) {
  uint32_t node = t;
  for (uint32_t d = 0; d <= n_pivots + 1; ++d) {
    if (node > n_pivots) return kTreeInvalid;   // an unlabelled pivot cell, a pivot outside the grid one hop ago, a label outside the list
    const uint32_t p = parent[node];
    if (p == kPathsPivotOob) return kTreeInvalid;   // this node's pivot lies outside the grid
    if (p == node) return d;
    node = p;
  }
  return kTreeInvalid;   // n_pivots + 2 hops without a self-loop: a cycle
}

// Entry t of the running-length table, for a pivot with 0 < depth[t] != kTreeInvalid once its parent's entry is final (the caller goes
// level by level; a root's entry is 0.0).  depth[t] valid makes parent[t] <= n_pivots and both pivots lie inside the grid.
VHP_PATHS_HD inline double tree_cum_entry(const uint32_t* parent, const int32_t* pivots_xy, const double* cum, uint32_t t) {
  const uint32_t p = parent[t];
  return cum[p] + paths_eval_d(pivots_xy[2 * (size_t)p], pivots_xy[2 * (size_t)p + 1], pivots_xy[2 * (size_t)t], pivots_xy[2 * (size_t)t + 1]);
}

// Builds a whole query's tables on one thread: the model of vhp_tree_tables (which spreads the same entries over a workgroup, the
// levels behind barriers), and what tests/tree_driver.cpp runs.  parent, depth, cum: n_pivots + 1 entries each.
VHP_PATHS_HD inline void tree_build_tables(const uint32_t* label, const int32_t* pivots_xy, uint32_t n_pivots, int nx, int ny, uint32_t* parent,
                                           uint32_t* depth, double* cum) {
  uint32_t deepest = 0;
  for (uint32_t t = 0; t <= n_pivots; ++t) parent[t] = paths_parent_entry(label, pivots_xy, t, nx, ny);
  for (uint32_t t = 0; t <= n_pivots; ++t) {
    depth[t] = tree_depth_entry(parent, n_pivots, t);
    cum[t] = 0.0;
    if (depth[t] != kTreeInvalid && depth[t] > deepest) deepest = depth[t];
  }
  for (uint32_t level = 1; level <= deepest; ++level)
    for (uint32_t t = 0; t <= n_pivots; ++t)
      if (depth[t] == level) cum[t] = tree_cum_entry(parent, pivots_xy, cum, t);
}

// One cell's result: what vhp_reconstruct_path from (x, y) reports, (x, y) inside the grid and `label` its label.  Returns true where
// that call returns VHP_OK (or VHP_ERR_TOO_LARGE: the caller's cap decides) with *n_path and *length the host's; false where it returns
// VHP_ERR_ARG, with the length field's filler: *length = -1.0, *n_path = 0.  depth, cum and pivots_xy may be LDS or global memory.
VHP_PATHS_HD inline bool tree_cell(uint32_t label, int x, int y, uint32_t n_pivots, const uint32_t* depth, const double* cum,
                                   const int32_t* pivots_xy, uint32_t* n_path, double* length) {
  *n_path = 0;
  *length = -1.0;
  if (label > n_pivots) return false;
  const uint32_t d = depth[label];
  if (d == kTreeInvalid) return false;
  *n_path = d + 2;
  *length = cum[label] + paths_eval_d(pivots_xy[2 * (size_t)label], pivots_xy[2 * (size_t)label + 1], x, y);
  return true;
}

// One goal's path: vhp_reconstruct_path(..., x, y, path_xy, cap, n_path, length) on a query with results.  label: the query's nx * ny
// labels; parent, depth, cum: its tables.  path_xy: cap points of room, or null (counts and length only, cap ignored, never
// kPathsErrTooLarge).  The points go straight into place, end first from slot n - 1 down: n = depth + 2 is known before the first one.
// *n_path and *length are the host's on kPathsOk and kPathsErrTooLarge and 0 on kPathsErrArg and kTreeErrEndOob (where the host leaves
// its outputs alone).  Nothing is written to path_xy unless the status is kPathsOk.
VHP_PATHS_HD inline int tree_goal_path(const uint32_t* label, const uint32_t* parent, const uint32_t* depth, const double* cum,
                                       const int32_t* pivots_xy, uint32_t n_pivots, int nx, int ny, int x, int y, int32_t* path_xy, uint32_t cap,
                                       uint32_t* n_path, double* length) {
  *n_path = 0;
  *length = 0.0;
  if (x < 0 || y < 0 || x >= nx || y >= ny) return kTreeErrEndOob;
  uint32_t t = label[(size_t)x + (size_t)y * nx];
  uint32_t n;
  double len;
  if (!tree_cell(t, x, y, n_pivots, depth, cum, pivots_xy, &n, &len)) return kPathsErrArg;
  *n_path = n;
  *length = len;
  if (!path_xy) return kPathsOk;
  if (n > cap) return kPathsErrTooLarge;
  path_xy[2 * (size_t)(n - 1)] = x;
  path_xy[2 * (size_t)(n - 1) + 1] = y;
  // depth[t] valid: the n - 1 nodes t, parent[t], ... are all <= n_pivots, and the last one is the root
  for (uint32_t k = n - 1; k > 0; --k) {
    path_xy[2 * (size_t)(k - 1)] = pivots_xy[2 * (size_t)t];
    path_xy[2 * (size_t)(k - 1) + 1] = pivots_xy[2 * (size_t)t + 1];
    t = parent[t];
  }
  return kPathsOk;
}

}  // namespace vhp
