// vhp_launch_plan.hpp -- how the pool sweep (vhp_pool.hip) and the latency sweep (vhp_lat.hip) are launched: pure functions of the
// launch, as vhp_choice.hpp is of which kernel runs.  Host code without a HIP header (with -DVHP_SIM the host compiler takes it):
// tests/test_launch_plans.py pins plan_pool and plan_lat against tests/golden/launch_plans.json, and the simulator (tests/sim) opens a
// launch with the launcher's own first round.  (The sizes of a pool-sweep launch's scratch: vhp_pool_scratch.hpp.)
// Every constant is a measurement; the comment beside it says which.
#pragma once
#include <cstddef>

#include "../../include/vhp.h"
#include "vhp_band.hpp"

namespace vhp {

constexpr size_t kLdsLimit = 160 * 1024;  // LDS of a CU: what one workgroup of either kernel may ask for

namespace pool {

// One persistent workgroup per CU; every wavefront is a Worker.  kWaves wavefronts: three per SIMD, 168 vector registers each
// (the builds use 121 and 114).
#ifndef VHP_POOL_WAVES
#define VHP_POOL_WAVES 12
#endif
constexpr int kWaves = VHP_POOL_WAVES;
// the build for widths that are not a multiple of 8: its tiles are three windows (12.8 KB a wavefront), nine wavefronts fit the LDS
#ifndef VHP_POOL_WAVES_ANYW
#define VHP_POOL_WAVES_ANYW 9
#endif
constexpr int kWavesAny = VHP_POOL_WAVES_ANYW;

// The latency sweep: one workgroup per unit (octant of a quadrant of a source); strip p is wavefront p mod kLatWaves's.  Eight
// wavefronts: two per SIMD, 256 vector registers each (a window keeps its 17 + 16 operands and the 16 pairs of its tile read-out in
// registers).
#ifndef VHP_LAT_WAVES
#define VHP_LAT_WAVES 8
#endif
constexpr int kLatWaves = VHP_LAT_WAVES;

#ifdef VHP_LAT_STRIPS  // A/B builds only: the sweep in strips of rows (vhp_lat.hpp), what the kernel was until round 6
template <typename OutT, bool ODD, bool MULTI = false> using LatWorkerT = LatWorker<OutT, ODD>;
#else
template <typename OutT, bool ODD, bool MULTI = false> using LatWorkerT = BandWorker<OutT, ODD, MULTI>;
#endif
constexpr int kLatTilePitch = LatWorkerT<double, false>::kTilePitch;
constexpr int kLatOrderPerThread = 2;  // units a thread of vhp_lat_order sorts (256 sources)

}  // namespace pool

// ---- the pool sweep ------------------------------------------------------------------------------------------------------------
// the vhp_set_option keys "pool_<member>" (0 / -1: automatic)
struct PoolOpts {
  int contexts = 0;      // units a workgroup holds at once
  int claim_ahead = -1;  // steps by which a strip is claimed ahead of the strip below's progress (-1: automatic)
  int heads = 0;         // contexts that pull from the head of the sorted queue
  int tail_pct = 0;      // share of the units (by count, smallest first) that the filler contexts may take from the small end
  int early_ctx = 0, late_pct = 0;  // contexts >= early_ctx open once late_pct % of the units are taken (0: all open)
  int busy_cap = 0;      // a workgroup takes another unit only while fewer wavefronts than this are sweeping (0: no cap)
  int static_round = 2;  // every context's first unit by workgroup index, no pull (vhp_pool.hpp Args::static_round; 2: odd head
                         // contexts count down, Args::static_snake); 0: every unit pulled
};

struct PoolPlan {
  bool ok;            // false: not even one context fits the LDS
  int n_ctx, waves;   // contexts (units a workgroup holds at once) and wavefronts of a workgroup
  size_t lds_bytes;
  int n_head, tail_limit, early_ctx, late_after, claim_ahead, busy_cap;  // vhp_pool.hpp Args
  bool static_round, static_snake;
  unsigned long long queue0;  // where the launch starts pulling (vhp_pool_order writes it)
};

struct PoolShape { int n_ctx; size_t lds; };
// as many contexts (units a workgroup holds at once) as asked for (default 4) that fit the LDS
// Measured (tools/ab_libs.py on one buffer, final launch order): 256 sources at 1000^2, 2 / 3 / 4 / 5 contexts 0.69 / 0.67-0.70 /
// 0.74 / 0.77 ms; 128 sources at 2048^2, 1 / 2 / 3 contexts 1.25 / 1.38 / 1.41 ms; at 4096^2 1 / 2: 3.88 / 4.80 ms -- units that
// large (a 4096^2 octant is 67 MB, 64 strips) keep every wavefront busy by themselves and only lose to a neighbour.
inline PoolShape pool_shape(int nx, int ny, int force_ctx, bool anyw) {
  PoolShape s;
  // Round 4 (non-temporal stores, strips claimed ahead; 128 sources, 1 / 2 / 3 contexts, ms): 1280^2 0.617 / 0.538 / 0.561; 1536^2 0.771 /
  // 0.741 / 0.772; 1792^2 0.933 / 0.956 / 1.005; 2048^2 1.106 / 1.189 / 1.233; 3072^2 (64 sources) 1.463 / 1.569 / 1.659; 4096^2 3.46 / 4.18 /
  // 4.35; 1024^2 (256 sources) - / 0.624 / 0.608: three up to 1024, two up to 1664, one above.
  const int maxdim = nx > ny ? nx : ny;
  s.n_ctx = force_ctx > 0 ? force_ctx : (maxdim > 1664 ? 1 : maxdim > 1024 ? 2 : 3);
  if (s.n_ctx > 16) s.n_ctx = 16;
  for (;; --s.n_ctx) {
    s.lds = (size_t)(anyw ? pool::make_layout(pool::kWavesAny, s.n_ctx, nx, ny, pool::kTStrideAny) : pool::make_layout(pool::kWaves, s.n_ctx, nx, ny)).total * 8;
    if (s.lds <= kLdsLimit || s.n_ctx == 1) break;
  }
  return s;
}

// The first unit of every context by workgroup index, the queue behind them (Args::static_round): only when every context is open from
// the start and every one of them finds a unit.
inline bool pool_static_round_ok(bool mode_on, int early_ctx, int n_ctx, int n_units, int n_groups) {
  return mode_on && early_ctx >= n_ctx && (long long)n_units >= (long long)n_ctx * n_groups;
}
// ... and the queue word behind that round: units taken from the head (low word) and from the tail (high word)
inline unsigned long long pool_queue0(int n_head, int n_ctx, int n_groups) {
  return (unsigned long long)(n_head * n_groups) | ((unsigned long long)((n_ctx - n_head) * n_groups) << 32);
}

// anyw: pool_needs_anyw<OutT>(...) of the launch's output (it needs the pointer)
inline PoolPlan plan_pool(int nx, int ny, int n_src, int n_cus, bool anyw, const PoolOpts& o) {
  PoolPlan p;
  const PoolShape sh = pool_shape(nx, ny, o.contexts, anyw);
  const int n_units = n_src * pool::kUnits;
  p.ok = sh.lds <= kLdsLimit;
  p.n_ctx = sh.n_ctx;
  p.lds_bytes = sh.lds;
  p.waves = anyw ? pool::kWavesAny : pool::kWaves;
  p.busy_cap = o.busy_cap > 0 ? o.busy_cap : p.waves;
  // two contexts take the largest units left, the others the smallest (0.75 against 0.78 ms with one head at 1000^2)
  p.n_head = o.heads > 0 ? o.heads : (sh.n_ctx >= 3 ? 2 : 1);  // (all three from the head: 0.51 / 0.70 ms on two boxes, this: 0.53 / 0.67)
  if (p.n_head > sh.n_ctx) p.n_head = sh.n_ctx;
  p.tail_limit = (int)((long long)n_units * (o.tail_pct > 0 ? o.tail_pct : 15) / 100);  // (100 / 50 / 25 / 15 %: 0.56 / 0.55 / 0.53 / - and - / - / - / 0.67 ms on two boxes; round 4, with non-temporal stores: 5 / 15 / 30 / 60 %: 0.580 / 0.608 / 0.608 / 0.616 ms on a slow buffer, level on a fast one -- within the noise of 1-2 %)
  p.early_ctx = o.early_ctx > 0 ? o.early_ctx : sh.n_ctx;
  p.late_after = (int)((long long)n_units * (o.late_pct > 0 ? o.late_pct : 50) / 100);
  // measured (tools/ab_slowfast.py, ab_libs.py; 0 / 16 / 32 / 48 / 64 steps): C3 on a fast buffer 0.485 / 0.468 / 0.463 / 0.461 / 0.460 ms, on a
  // slow one 0.583 / 0.582 / 0.597 / 0.589 / 0.591 (bound by the memory there); C5 3.567 / 3.483 / 3.476 / 3.474 / 3.482; 128 sources at
  // 2048^2 1.316 / - / 1.277 / - / 1.238; 512 at 512^2 0.445 / - / 0.419 / - / 0.416
  p.claim_ahead = o.claim_ahead >= 0 ? o.claim_ahead : 48;
  p.static_snake = o.static_round >= 2;
  p.static_round = pool_static_round_ok(o.static_round != 0, p.early_ctx, sh.n_ctx, n_units, n_cus);
  p.queue0 = p.static_round ? pool_queue0(p.n_head, sh.n_ctx, n_cus) : 0ull;
  return p;
}

inline bool pool_supported(int nx, int ny) {
  if (nx <= 0 || ny <= 0 || nx > VHP_MAX_SIDE || ny > VHP_MAX_SIDE) return false;
  return pool_shape(nx, ny, 0, false).lds <= kLdsLimit && pool_shape(nx, ny, 0, true).lds <= kLdsLimit;
}

// ---- the latency sweep ---------------------------------------------------------------------------------------------------------
#ifndef VHP_LAT_HALVES_MIN_SIDE
#define VHP_LAT_HALVES_MIN_SIDE 1024
#endif
// Workgroups per unit of a latency-sweep launch (LatArgs::halves; vhp_band.hpp BandWorker).  One up to 1024 cells a side: an octant
// has at most 16 bands there, and what bands 8-15 gain by not waiting for the sweepers of bands 0-7 the hand-over through global
// memory takes back (measured at 1000^2: 117.8 / 118.4 us over eight source positions).  Above: two up to 2048, four up to 4096, eight
// beyond -- an octant of P bands is swept in rounds of 8 x that number, and every round waits for the one before (8192^2, one source:
// 3.47 ms with one workgroup per unit, 1.92 with two, 1.18 with four), halved until the launch is at most twice the chip.  (asked: vhp_set_option "lat_workgroups", 1 / 2 / 4 / 8, for
// measurements and tests; 0: by the size.)
inline int lat_halves(int n_src, int nx, int ny, int n_cus, int asked) {
  const int cus = n_cus > 0 ? n_cus : 256, side = nx > ny ? nx : ny;
  const int want = asked > 0 ? asked : side > 4 * VHP_LAT_HALVES_MIN_SIDE ? 8 : side > 2 * VHP_LAT_HALVES_MIN_SIDE ? 4 : side > VHP_LAT_HALVES_MIN_SIDE ? 2 : 1;
  int h = 1;
  // (up to twice as many workgroups as CUs -- a launch of more workgroups than CUs is safe, BandWorker::run, and a unit's later
  // workgroups start while its first ones are at their first bands: 16 sources at 4096^2 1265 us with two workgroups per unit, 1193 with
  // four; 8 at 8192^2 2718 with four, 2447 with eight; a number that was asked for is taken as it is)
  // (... beyond two that fit: 32 sources at 1536^2 take 280 us with one workgroup per unit and 316 with two on twice the chip)
  while (2 * h <= want && 2 * h <= 8 && (asked > 0 || 2 * h * pool::kUnits * n_src <= (h >= 2 ? 2 : 1) * cus)) h *= 2;
  return h;
}
inline size_t lat_lds_bytes(int nx, int ny) { return (size_t)pool::make_layout(pool::kLatWaves, 1, nx, ny, pool::kLatTilePitch).total * 8; }

// which of BatchArgs::d_lat_order and the members of LatLaunch a launch sets
struct LatFlags {
  bool d_lat_order = false, pivot_rec = false, src_index = false, slot_base = false, map_idx = false, planner_dev = false;
};

struct LatPlan {
  bool ok;                // false: the workgroup's LDS does not fit
  bool odd;               // the odd-pitch build (lat_needs_odd of the launch's output)
  int halves;             // workgroups per unit (a planner iteration launches one whatever this says: its grid is the eight octants)
  size_t lds_bytes;
  bool use_order_kernel;  // vhp_lat_order ahead of the sweep
};

// odd: lat_needs_odd<OutT>(...) of the launch's output; asked: vhp_set_option "lat_workgroups"
inline LatPlan plan_lat(int nx, int ny, int n_src, int n_cus, bool odd, int asked_workgroups, const LatFlags& f) {
  LatPlan p;
  p.odd = odd;
  p.halves = lat_halves(n_src, nx, ny, n_cus, asked_workgroups);
#if defined(VHP_LAT_STRIPS) || defined(VHP_EXP_ONE_KERNEL)  // (A/B and compile-time experiments: built for one workgroup per unit)
  p.halves = 1;
#endif
  p.lds_bytes = lat_lds_bytes(nx, ny);
  p.ok = p.lds_bytes <= kLdsLimit;
  // more workgroups than the chip holds at once: the long units first
  p.use_order_kernel = p.halves == 1 && n_src * pool::kUnits > (n_cus > 0 ? n_cus : 256) && n_src * pool::kUnits <= 1024 * pool::kLatOrderPerThread &&
                       f.d_lat_order && !f.pivot_rec && !f.src_index && !f.slot_base && !f.planner_dev;
  return p;
}

// The timestamps a launch writes from inside its kernels when it is given a slot for them (vhp_stamps.hpp): one begin entry by its
// one-workgroup pre-kernel, or one per workgroup where it has none, and one end entry per workgroup of its sweep kernel.
struct StampCounts {
  int n_begin, n_end;
};
inline StampCounts pool_stamp_counts(int n_cus) { return {1, n_cus > 0 ? n_cus : 256}; }   // (vhp_pool_order, then one workgroup per CU)
inline StampCounts lat_stamp_counts(const LatPlan& p, int n_src) {
  const int groups = n_src * pool::kUnits * p.halves;
  return {p.use_order_kernel ? 1 : groups, groups};
}

inline bool lat_supported(int nx, int ny) {
  if (nx <= 0 || ny <= 0 || nx > VHP_MAX_SIDE || ny > VHP_MAX_SIDE) return false;
  // (a y-major workgroup keeps its quadrant's diagonal where an x-major one has its tiles)
  return lat_lds_bytes(nx, ny) <= kLdsLimit && (size_t)pool::kLatWaves * pool::kXRows * pool::kTStride >= (size_t)(nx < ny ? nx : ny);
}

}  // namespace vhp
