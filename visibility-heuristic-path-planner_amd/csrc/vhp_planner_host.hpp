// vhp_planner_host.hpp -- what the planner's three solves (plain, speculative, batch) decide on the host before and after their loops:
// the validity checks of a query, the loop-end messages, scale_ and the capacity of the pivot list.
// Host-only and free of HIP: tests/test_planner_host.py compiles it with the host compiler (tests/planner_host_driver.cpp) and pins it
// against the oracle.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "vhp.h"

namespace vhp {

struct QueryCheck {
  int code;          // VHP_OK, or the reference's code for the first check that fails
  const char* msg;   // its message (null when the query passes)
};

inline bool planner_in_bounds(int nx, int ny, int x, int y) { return (size_t)x < (size_t)nx && (size_t)y < (size_t)ny; }

// The four validity checks of solve(), in the reference's order (solver.cpp:89-116).  occ_start / occ_end: the occupancy complement at
// the two points (0: blocked), supplied by the caller; where a point is out of bounds neither is looked at.
inline QueryCheck planner_check_query(int nx, int ny, int sx, int sy, int ex, int ey, uint8_t occ_start, uint8_t occ_end) {
  if (!planner_in_bounds(nx, ny, sx, sy)) return {VHP_ERR_START_OOB, "Start point is out of bounds."};
  if (!planner_in_bounds(nx, ny, ex, ey)) return {VHP_ERR_END_OOB, "End point is out of bounds."};
  if (!occ_start) return {VHP_ERR_START_OCCUPIED, "Start point is not valid (occupied)"};
  if (!occ_end) return {VHP_ERR_END_OCCUPIED, "End point is not valid (occupied)"};
  return {VHP_OK, nullptr};
}

// What a solve says when its loop ends without reaching the end point (null for every other status).
inline const char* planner_status_message(int status) {
  if (status == VHP_ERR_MAX_ITER) return "Max iters hit. Solution could not be found. Try lowering visibility threshold.";
  if (status == VHP_ERR_NOTHING_LIT) return "no cell reached the visibility threshold";
  return nullptr;
}

// (volatile: the sum is rounded to a double and the root taken of that double at run time, as the reference's build does)
inline double planner_scale(int nx, int ny) {
  volatile double q = (double)((size_t)ny * ny + (size_t)nx * nx);
  return std::sqrt(q);  // scale_, solver.cpp:49
}

// int32 entries of a pivot list for max_iter iterations: lightSources_[0 .. max_iter + 1] as (x, y), plus `extra` pivots (the
// speculative solve's runner-ups past the end: kSpecMaxK).
inline size_t planner_pivot_ints(uint64_t max_iter, int extra = 0) { return 2 * (size_t)(max_iter + 2 + (uint64_t)extra); }

}  // namespace vhp
