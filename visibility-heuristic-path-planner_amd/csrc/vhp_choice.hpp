// vhp_choice.hpp -- which kernel sweeps a batch, and the front sweep's launch shape: one pure function of the launch.
// Host-only and free of HIP: tests/test_kernel_choice.py compiles it with the host compiler and pins it against
// tests/golden/kernel_choice.json.  Every threshold is a measured crossover; the measurements are in DESIGN.md section 0,
// "Kernel choice: the measurements behind each rule", under the rule's name.
#pragma once

#include <algorithm>
#include <climits>

namespace vhp {

// the vhp_set_option keys that steer the choice (0 / -1: automatic)
struct ChoiceOpts {
  int kernel = 0;         // 0 auto, 1 front sweep, 3 pool sweep, 4 latency sweep
  int rows_per_lane = 0;  // R: 1, 2 or 4
  int strips = 0;         // W: 1..8
  int multi = 0;          // 1: the multi-round build
  int slide = -1;         // 0 / 1: y-major column grid slid onto 128-byte lines
  int pack = 0;           // 1: short quadrants packed into one workgroup
};

struct ChoiceIn {
  int nx = 0, ny = 0, n_src = 0, n_cus = 256;
  bool f64 = true;
  ChoiceOpts opt;
  // evaluated by the caller: lat_supported, pool_supported (vhp_launch_plan.hpp), lat_scratch_bytes(n_src) <= 2 GiB (vhp_lat.hip)
  bool lat_ok = false, pool_ok = false, lat_scratch_fits = false;
};

// kernel: 1 front sweep (vhp_sweep.hip.h), 3 pool sweep (vhp_pool.hpp), 4 latency sweep (vhp_lat.hpp).
// R, W, multi: the front sweep's shape, filled whatever the kernel (the planner builds its front sweep from it); slide: kernel 1's.
struct SweepPlan {
  int kernel;
  int R, W;
  bool multi;
  int slide;
};

namespace choice {

// ladders of thresholds: the first row whose side is not exceeded (the last row has no limit)
struct Step { int max_side, value; };
struct ShapeStep { int max_side, R, W; };
template <typename Row, int N>
constexpr const Row& row_for(const Row (&t)[N], int side) {
  for (const Row& r : t)
    if (side <= r.max_side) return r;
  return t[N - 1];
}

// Rule "latency sweep beyond one octant per CU": the latency sweep wins up to this many quarters of a round of octants
// (n_cus / 8 sources), its units in order of length (profiles/r06_exp_lat_beyond_one_octant_per_cu.txt).
constexpr Step kLatQuarters[] = {{256, 16}, {640, 12}, {896, 10}, {1024, 8}, {1280, 5}, {INT_MAX, 4}};
// Rule "latency sweep, other widths": the latency sweep wins further there (tools/kernel_choice_other_widths.py).
constexpr Step kLatQuartersAnyW[] = {{256, 12}, {1280, 16}, {INT_MAX, 4}};
// Rule "pool sweep, widths a multiple of 8": the pool sweep wins from this many sources, from side 448
// (profiles/r05_front_vs_pool_multiples_of_8.txt).
constexpr Step kPoolMinSrc[] = {{575, 96}, {767, 48}, {1024, 33}, {2560, 24}, {INT_MAX, 17}};
// Rule "pool sweep, other widths": its ANYW build wins from this many sources, from side 450
// (profiles/r05_front_vs_pool_plain_front_stores.txt).
constexpr Step kPoolMinSrcAnyW[] = {{600, 256}, {768, 128}, {1100, 64}, {INT_MAX, 24}};
// Rule "front sweep shape": R rows per lane, W strips per octant (tools/ab_libs.py, tools/small_grid_shapes.py).
constexpr ShapeStep kShape[] = {{64, 1, 1}, {128, 2, 1}, {256, 1, 4}, {512, 2, 4}, {1024, 2, 8}, {INT_MAX, 4, 8}};

inline bool use_lat(const ChoiceIn& in, int side) {
  const ChoiceOpts& o = in.opt;
  if (o.kernel != 0 && o.kernel != 4) return false;
  if (!in.lat_ok) return false;
  if (o.kernel == 4) return in.n_src <= 256 && in.lat_scratch_fits;
  // (a caller that sets a launch shape of the front sweep is asking for the front sweep)
  if (o.rows_per_lane || o.strips || o.multi || o.slide >= 0 || o.pack) return false;
  const bool w8 = (in.nx & 7) == 0;
  // Rule "latency sweep, 17-32 sources on large grids": the pool sweep wins where the octants are back to one workgroup each
  // (profiles/r06_exp_workgroups_per_unit.txt).
  if (w8 && in.pool_ok) {
    if (in.n_src > 16 && side > 2560) return false;
    if (in.n_src >= 28 && side > 1792) return false;
  }
  const int cap = in.n_cus / 8 * (w8 ? row_for(kLatQuarters, side) : row_for(kLatQuartersAnyW, side)).value / 4;
  // (the boundary lines of a launch -- 16 bytes per strip and step -- stay below two gigabytes: 32 sources at 8192^2 would take four)
  return in.n_src <= std::min(cap, 128) && in.lat_scratch_fits;
}

inline bool use_pool(const ChoiceIn& in, int side) {
  const ChoiceOpts& o = in.opt;
  if (o.kernel == 1 || o.kernel == 4) return false;
  if (!in.pool_ok) return false;
  if (o.kernel == 3) return true;
  if ((in.nx & 7) != 0) return side >= 450 && in.n_src >= row_for(kPoolMinSrcAnyW, side).value;
  return side >= 448 && in.n_src >= row_for(kPoolMinSrc, side).value;
}

}  // namespace choice

inline SweepPlan plan_sweep(const ChoiceIn& in) {
  const ChoiceOpts& o = in.opt;
  const int side = std::max(in.nx, in.ny);
  SweepPlan p;
  p.kernel = choice::use_lat(in, side) ? 4 : choice::use_pool(in, side) ? 3 : 1;
  int R = choice::row_for(choice::kShape, side).R, W = choice::row_for(choice::kShape, side).W;
  // Rule "front sweep, fp32 batches": one row per lane, 8 strips, from 256 sources on widths a multiple of 8 (round 1).
  if (!in.f64 && side > 256 && side <= 1024 && in.n_src >= 256 && (in.nx & 7) == 0) { R = 1; W = 8; }
  if (o.rows_per_lane) R = o.rows_per_lane;
  if (o.strips) W = o.strips;
  bool multi = W * 64 * R < side || o.multi;
  if (R == 2 && multi && W > 4) W = 4;  // that build is compiled for 8-wavefront workgroups
  if (!in.f64) {
    // fp32 fields: only the one-row-per-lane shape is built; as many strips as the rows need, up to 8, unless set or already
    // one row per lane (small and odd-width grids keep their small workgroups)
    if (!o.strips && R != 1) W = std::min(W * R, 8);
    R = 1;
    multi = W * 64 < side || o.multi;
  }
  p.R = R;
  p.W = W;
  p.multi = multi;
  // Rule "slide": pays in the store-bound regime, from 96 sources (many quadrants in flight).
  p.slide = o.slide >= 0 ? o.slide : in.n_src >= 96 ? 1 : 0;
  return p;
}

}  // namespace vhp
