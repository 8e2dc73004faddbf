// vhp_planner_cell.hpp -- what a planner step decides about ONE cell, written once for the device and for the host compiler (no HIP
// types: tests/planner_cell_driver.cpp builds it with g++ and runs whole steps through it): is the cell swept from this pivot at all,
// its distance terms, its heuristic, its place in the reference's push order and the order of two candidates for the next pivot.
// The epilogues of vhp_planner_dev.hip.h (the plain and batch solves) and vhp_planner.hip.h (the speculative solve, and the export of
// its last field) call these and nothing of their own for the same questions.
// Reference: src/visibilityBasedSolver.cpp:379-565 (updateVisibility), include/solver/visibilityBasedSolver.h:16-21, :112-115.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHP_CELL_FN __host__ __device__ __forceinline__
#else
#define VHP_CELL_FN inline
#endif

namespace vhp {

struct PlannerKey {
  unsigned long long h;     // bits of the heuristic (h >= 0, so the bit pattern orders like the value)
  unsigned long long rank;  // push order, lower = earlier
  int x, y;
};

VHP_CELL_FN bool key_less(const PlannerKey& a, const PlannerKey& b) {
  return a.h < b.h || (a.h == b.h && a.rank < b.rank);
}

// eval_d, visibilityBasedSolver.h:112-115: first product in double, second in int
VHP_CELL_FN double eval_d_dev(int ax, int ay, int bx, int by) {
  const int dx = ax - bx, dy = ay - by;
  return __builtin_sqrt((double)dx * dx + (double)(dy * dy));
}

// column 0 / row 0 are swept only when the pivot lies on them (the quadrants towards lower x / lower y stop one cell short
// of the border): a cell the pivot (sx, sy) does not sweep is neither united, labelled nor pushed, and whatever an earlier sweep left
// there in a field that is not cleared between pivots must not be read
VHP_CELL_FN bool planner_unswept(int sx, int sy, int x, int y) {
  return (x == 0 && sx > 0) || (y == 0 && sy > 0);
}

// the heuristic of a lit cell, solver.cpp:424-430, in the reference's association: g the cell's value in the union, d_end / d_parent
// its eval_d to the end and to the pivot that labelled it
VHP_CELL_FN double planner_h(double scale, double g, double d_end, double d_parent) {
  return (scale * g) + (d_end + d_parent);
}

// push-order rank of cell (x, y) for the pivot (sx, sy): quadrants in the order Q1..Q4,
// inside a quadrant the x offset is the outer loop and the y offset the inner one
// (solver.cpp:392-395 etc.); a cell several quadrants visit counts where it is first pushed.
VHP_CELL_FN unsigned long long push_rank(int nx, int ny, int sx, int sy, int x, int y) {
  const long long dx = x - sx, dy = y - sy;
  long long q, r;
  if (dx >= 0 && dy >= 0) { q = 0; r = dx * (ny - sy) + dy; }
  else if (dx < 0 && dy >= 0) { q = 1; r = (-dx) * (ny - sy) + dy; }
  else if (dy < 0 && (dx < 0 || (dx == 0 && sx >= 1))) { q = 2; r = (-dx) * (long long)sy + (-dy); }
  else { q = 3; r = dx * (long long)sy + (-dy); }
  (void)nx;
  return ((unsigned long long)q << 40) | (unsigned long long)r;
}

}  // namespace vhp
