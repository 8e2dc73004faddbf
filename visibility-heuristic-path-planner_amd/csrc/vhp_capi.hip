// vhp_capi.hip -- the C ABI of include/vhp.h over the HIP kernels (gfx950).
// No CPU fallback lives here: every compute entry point launches HIP kernels and
// fails with VHP_ERR_HIP when the device or the runtime is unusable.
#include "vhp.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "vhp_batch_launch.h"
#include "vhp_choice.hpp"
#include "vhp_sweep.hip.h"
#include "vhp_maps.hip.h"
#include "vhp_planner.hip.h"
#include "vhp_planner_batch.hip.h"
#include "vhp_paths.hip.h"
#include "vhp_tree.hip.h"
#include "vhp_queue.hip.h"
#include "vhp_raycast_launch.h"
#include "vhp_stamps.hpp"
#include "vhp_variant.hip.h"
#include "vhp_union.hip.h"

struct vhp_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  vhp::stamps::Last timed;  // what vhp_last_elapsed_ms reports: nothing, ev0 / ev1, or the stamps of a pool- or latency-sweep launch
  std::string err;

  int n_cus = 256;
  std::vector<void*> placed;   // buffers handed out by vhp_alloc_output
  vhp::DevBuf<unsigned> d_probe_counter;  // task counter of vhp_probe_stores
  double last_alloc_ms = 0.0;  // what the last vhp_alloc_output cost: wall time of the search ...
  unsigned long long last_alloc_peak_bytes = 0;  // ... and the device memory it held at its peak (vhp_alloc_output_cost)
  int opt_alloc_budget_pct = 25;  // vhp_alloc_output: share of the free device memory its candidates may hold at once
  vhp::PackedMaps map;         // the map of vhp_set_map (n == 1): its packed copies, with the diagonal maps where the latency sweep takes the grid
  vhp::DevBuf<uint8_t> d_occ;  // ... its uint8 form (kept for the planner's validation and packing)
  std::vector<uint8_t> h_occ;  // ... and that one's host copy when vhp_set_map brought it (empty after vhp_set_map_device)
  vhp::DevBuf<int> d_err;

  // grow-only scratch (vhp_devbuf.hpp: a failed grow leaves an empty buffer); first the host-buffer sweep entry points' (stage_batch)
  vhp::DevBuf<int32_t> d_src;
  vhp::DevBuf<void> d_out;
  vhp::DevBuf<double> d_bnd;     // boundary rows of multi-round sweeps (sides above W*64*R)
  vhp::DevBuf<int> d_order;      // launch order of the (source, quadrant) units (+ one int4 descriptor per workgroup)
  vhp::DevBuf<int> d_lat_order;  // launch order of the latency sweep's units where it launches more of them than the device has CUs
  vhp::DevBuf<int> d_pool;       // pool sweep: pull counter, unit order, diagonal lines, tagged boundary lines (zeroed when allocated)
  unsigned long long pool_epoch = 0x5A17000000000000ull;  // tag of the last pool launch
  bool timing = false;      // every sweep launch is timed (vhp_timing): by the stamps its kernels write, else by an event pair around it
  struct TimedLaunch {      // ... one or the other
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    vhp::stamps::Launch st;
  };
  std::vector<TimedLaunch> timed_launches;  // oldest first
  std::vector<std::pair<hipEvent_t, hipEvent_t>> event_pool;  // recycled pairs: no hipEventCreate inside a timed loop
  // the stamps (vhp_stamps.hpp): slot 0 for the launches with vhp_timing off, then vhp_timing's ring; allocated by vhp_create and
  // vhp_timing, never inside a launch
  vhp::DevBuf<vhp::stamps::Entry> d_stamps;
  std::vector<vhp::stamps::Entry> h_stamps;  // their host copy, slot by slot
  vhp::stamps::Ring ring;
  int clock_khz = 0;        // rate of the clock the stamps read (hipDeviceAttributeWallClockRate); 0: no stamps, events everywhere

  // launch-shape overrides (vhp_set_option); 0 / -1 = automatic
  int opt_rows_per_lane = 0;  // R: 1, 2 or 4
  int opt_strips = 0;         // W: 1..8
  int opt_multi = 0;          // 1: force the multi-round build
  int opt_slide = -1;         // 0 / 1: y-major column grid slid onto 128-byte lines
  int opt_pack = 0;           // 1: pack short quadrants into one workgroup
  int opt_lat_workgroups = 0; // latency sweep: workgroups per octant (0 automatic, 1 / 2 / 4 / 8: vhp_launch_plan.hpp lat_halves)
  int opt_kernel = 0;         // 0 auto, 1 front sweep (vhp_sweep_fronts), 3 pool sweep (vhp_pool), 4 latency sweep (vhp_lat); 2 was the streaming sweep (retired in round 4)
  int last_kernel = 0;         // what the last batch sweep launched: 1 front sweep, 3 pool sweep, 4 latency sweep
  long long opt_field_stride = 0;  // device-pointer batch sweeps: elements from one field to the next (0: nx * ny, packed)
  vhp::PoolOpts opt_pool;   // pool sweep: the "pool_*" keys (vhp_launch_plan.hpp plan_pool)

  vhp::PlannerState pl;  // device-resident planner state
  vhp::SpecState spec;   // field cache of the speculative planner
  vhp::BatchState batch; // the batch planner's queries (vhp_planner_solve_batch), apart from pl
  int opt_planner_batch_group = 0;  // queries per group of a batch solve at most (0: automatic, planner_batch_group_size)
  vhp::QueueScratch qs;  // scratch of the queue-variant sweep

  // the stack of maps of vhp_set_maps (vhp_sweep_maps_batch): state of its own, apart from the single map above; its diagonal maps are
  // built by the first planner batch on the stack that takes the latency sweep (vhp_planner_solve_maps_batch) and kept until the stack goes
  vhp::PackedMaps maps;
  vhp::DevBuf<int32_t> d_map_idx;   // host-buffer form's slice of map indices (grow-only)
  vhp::DevBuf<uint64_t> d_inflate;  // vhp_inflate_map / vhp_inflate_maps: the inflated packed copies before they replace the old ones (grow-only)
  vhp::BatchState maps_batch;       // the planner batch on the stack (vhp_planner_solve_maps_batch): apart from `batch` and pl
  vhp::PathsScratch paths;          // scratch and staging of the path calls (vhp_planner_path, vhp_planner_[maps_]batch_paths)
  vhp::TreeScratch tree;            // tables and staging of the tree calls (vhp_planner_length_fields, vhp_planner_goal_paths)
};

namespace {

// Every entry point runs on the context's device and leaves the caller's current device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (device, function) pair, not to a context: two contexts on
// one device share it.  Kept process-wide and monotonic -- the attribute is never set to a smaller value than before, so a
// context that raised it for a large grid is not undercut by another context's small one.
hipError_t raise_lds_limit(vhp_ctx* c, const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> raised;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = raised[{c->device, fn}];
  if (have >= bytes) return hipSuccess;
  hipError_t r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (r == hipSuccess) have = bytes;
  return r;
}

int fail(vhp_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define VHP_HIP(call)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, VHP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
  } while (0)

#define VHP_ON_DEVICE(ctx)                   \
  DeviceGuard device_guard_((ctx)->device); \
  if (!device_guard_.ok) return fail((ctx), VHP_ERR_HIP, "hipSetDevice failed")

// Map 0 of p; a sweep on a stack moves to map k by k times maps_stack's strides.
vhp::DevMap dev_map(const vhp::PackedMaps& p) {
  vhp::DevMap m;
  m.rows = p.rows.get();
  m.cols = p.cols.get();
  m.recip = p.recip.get();
  m.wpr = p.wpr;
  m.wpc = p.wpc;
  m.nx = p.nx;
  m.ny = p.ny;
  m.bnd = nullptr;
  m.bnd_len = 0;
  m.slide = 0;  // set per launch (launch_sweep_t)
  return m;
}

vhp::MapStack maps_stack(const vhp::PackedMaps& p, const int32_t* d_map_idx) {
  return {d_map_idx, p.n, vhp::map_rows(p, 1) - vhp::map_rows(p, 0), vhp::map_cols(p, 1) - vhp::map_cols(p, 0)};
}

void free_map(vhp_ctx* c) {
  c->d_occ.reset();
  c->map = vhp::PackedMaps{};
  c->h_occ.clear();
  c->pl.h_occ = nullptr;
  vhp::planner_free(c->pl);
  c->spec = vhp::SpecState{};
  vhp::batch_free(c->batch);
  c->qs = vhp::QueueScratch{};
}

void free_maps(vhp_ctx* c) {
  c->maps = vhp::PackedMaps{};
  vhp::batch_free(c->maps_batch);
}

// How an internal launch writes its fields and whether vhp_timing times it.  The entry point passes it down; nothing parks it on the
// context around a call.  The default is the planner loops': packed fields, and no per-launch event pairs (vhp_timing times sweep
// launches, and a loop enqueues launches past its end that return at once -- they would fill the pool with pairs that time nothing).
struct LaunchOpts {
  long long field_stride = 0;  // elements from one field to the next (0: nx * ny, packed)
  bool timed = false;
  // a pool- or latency-sweep launch that writes its own timestamps: the slot the entry point took for it (take_stamp_slot); the launch
  // fills in its tag.  Null: timed by events, if at all.
  vhp::stamps::Launch* stamp = nullptr;
};

// -DVHP_TIMING_STAMPS=0: no launch writes timestamps, event records time every one of them (an A/B build, tools/ab_libs.py)
#ifndef VHP_TIMING_STAMPS
#define VHP_TIMING_STAMPS 1
#endif

// The library's timing events -- the context's ev0 / ev1 and vhp_timing's pairs -- carry no system-scope fence.  A plain hipEvent
// releases to the system when it is recorded: a cache write-back and invalidate between one launch's sweep and the next launch's
// order kernel, twice per pair.  Nothing needs it here: every wait on one of these events (vhp_timing_collect, vhp_last_elapsed_ms,
// vhp_probe_stores) is followed by hipEventElapsedTime and by no read of memory; what the host or another stream reads, it reads
// behind hipStreamSynchronize, a copy or a kernel boundary, which order memory by themselves.  The events something is read on the
// strength of (the planners' poll events, the multi-device `done` events) are created elsewhere and keep their fence.
// (VHP_TIMING_EVENT_FLAGS: hipEventReleaseToDevice or 0 for an A/B build, tools/ab_libs.py)
#ifndef VHP_TIMING_EVENT_FLAGS
#define VHP_TIMING_EVENT_FLAGS hipEventDisableSystemFence
#endif
hipError_t create_timing_event(hipEvent_t* e) { return hipEventCreateWithFlags(e, VHP_TIMING_EVENT_FLAGS); }

// A timed launch's events (else none): a recycled pair, or a new one.
using EventPair = std::pair<hipEvent_t, hipEvent_t>;
hipError_t acquire_events(vhp_ctx* c, bool timed, EventPair* ev) {
  *ev = {nullptr, nullptr};
  if (!timed) return hipSuccess;
  if (!c->event_pool.empty()) { *ev = c->event_pool.back(); c->event_pool.pop_back(); return hipSuccess; }
  if (create_timing_event(&ev->first) != hipSuccess) return hipErrorOutOfMemory;
  if (create_timing_event(&ev->second) == hipSuccess) return hipSuccess;
  (void)hipEventDestroy(ev->first);
  return hipErrorOutOfMemory;
}
// ... timed if the launch went out; back to the pool if it failed (a pair that was never recorded can never be waited for)
void release_events(vhp_ctx* c, const EventPair& ev, hipError_t launched) {
  if (!ev.first) return;
  if (launched == hipSuccess) c->timed_launches.push_back({ev, {}});
  else c->event_pool.push_back(ev);
}

// The stamps' device array for the ring as it is now: (re)allocated and zeroed, with its host copy.  Not inside a launch: hipMalloc
// and hipFree wait for the device.  A failure leaves no array, and with it no stamped launches.
hipError_t allocate_stamps(vhp_ctx* c) {
  hipError_t e = c->d_stamps.grow(c->ring.bytes());
  if (e == hipSuccess) e = hipMemsetAsync(c->d_stamps.get(), 0, c->ring.bytes(), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { c->d_stamps.reset(); return e; }
  c->h_stamps.assign(c->ring.bytes() / sizeof(vhp::stamps::Entry), vhp::stamps::Entry{0, 0});
  return hipSuccess;
}

// The slot for the timestamps of a plain launch of n_src sources by the pool sweep (kernel 3) or the latency sweep (kernel 4): one
// of the ring's if the launch is timed, slot 0 if not; .slot = -1 where the launch is timed by events -- another kernel, no clock, a
// launch of more workgroups than a slot has entries for, the ring full.
vhp::stamps::Launch take_stamp_slot(vhp_ctx* c, int kernel, int n_src, bool timed) {
  vhp::stamps::Launch st;
  if (!VHP_TIMING_STAMPS || (kernel != 3 && kernel != 4) || c->clock_khz <= 0 || !c->d_stamps.get()) return st;
  const vhp::StampCounts sc = kernel == 4 ? vhp::lat_stamp_counts(vhp::plan_lat(c->map.nx, c->map.ny, n_src, c->n_cus, false, c->opt_lat_workgroups, {true}), n_src)
                                          : vhp::pool_stamp_counts(c->n_cus);
  if (!c->ring.fits(sc.n_begin, sc.n_end)) return st;
  st.slot = timed ? c->ring.take() : 0;
  st.n_begin = sc.n_begin;
  st.n_end = sc.n_end;
  st.stream = c->stream;
  return st;
}

// The host copy of the `count` slots from `first` on.
hipError_t copy_stamp_slots(vhp_ctx* c, int first, int count) {
  const size_t at = c->ring.slot_offset(first);
  return hipMemcpy(c->h_stamps.data() + at, c->d_stamps.get() + at, (size_t)count * vhp::stamps::slot_bytes(c->ring.groups()), hipMemcpyDeviceToHost);
}

// vhp_last_elapsed_ms's stamped launch, read: its stream synchronised, its entries copied and reduced (Last::kStamps -> kRead).
void read_last_stamps(vhp_ctx* c) {
  if (c->timed.state != vhp::stamps::Last::kStamps) return;
  const vhp::stamps::Launch l = c->timed.launch;
  vhp::stamps::Time t;
  const size_t at = c->ring.slot_offset(l.slot);
  if (hipStreamSynchronize(static_cast<hipStream_t>(l.stream)) == hipSuccess &&
      hipMemcpy(c->h_stamps.data() + at, c->d_stamps.get() + at, (size_t)(l.n_begin + l.n_end) * sizeof(vhp::stamps::Entry), hipMemcpyDeviceToHost) == hipSuccess)
    t = vhp::stamps::reduce(c->h_stamps.data() + at, l, c->clock_khz);
  else
    (void)hipGetLastError();
  c->timed.read(l.tag, t);
}

// What sweeps a batch of n_src sources on m's grid with the context's options (vhp_choice.hpp), or with `kernel` in place of the option.
vhp::SweepPlan plan_for_grid(const vhp_ctx* c, const vhp::PackedMaps& m, int n_src, bool f64, int kernel = 0) {
  const bool lat_ok = vhp::lat_supported(m.nx, m.ny);
  return vhp::plan_sweep({m.nx, m.ny, n_src, c->n_cus, f64,
                          {kernel ? kernel : c->opt_kernel, c->opt_rows_per_lane, c->opt_strips, c->opt_multi, c->opt_slide, c->opt_pack}, lat_ok,
                          vhp::pool_supported(m.nx, m.ny), lat_ok && vhp::lat_scratch_bytes(n_src, m.nx, m.ny) <= ((size_t)2 << 30)});
}

// ... on the context's map, and on its stack of maps: always the front sweep there (vhp_sweep_fronts_maps)
vhp::SweepPlan plan_for(const vhp_ctx* c, int n_src, bool f64) { return plan_for_grid(c, c->map, n_src, f64); }
vhp::SweepPlan plan_for_maps(const vhp_ctx* c, int n_src, bool f64) { return plan_for_grid(c, c->maps, n_src, f64, 1); }

// The planner's sweeps of n_src sources: the plan, and the front sweep's shape and round scratch (n_workgroups) from it.
hipError_t plan_planner(vhp_ctx* ctx, vhp::DevMap& pm, int n_src, size_t n_workgroups, vhp::SweepPlan* plan) {
  *plan = plan_for(ctx, n_src, true);
  hipError_t e = vhp::attach_round_scratch(pm, plan->W * 64 * plan->R, n_workgroups, ctx->d_bnd);
  if (e != hipSuccess) return e;
  ctx->pl.R = plan->R;
  ctx->pl.W = plan->W;
  ctx->pl.multi = plan->multi;
  ctx->pl.raise_lds = [ctx](const void* fn, size_t bytes) { return raise_lds_limit(ctx, fn, bytes); };
  ctx->last_kernel = plan->kernel == 4 ? 4 : 1;  // (vhp_last_sweep_kernel after a solve: what swept its iterations)
  return hipSuccess;
}

// The front sweep: a workgroup sweeps one quadrant with 2*W wavefronts (W strips per octant) and R rows/columns per lane;
// fronts longer than W*64*R are swept in rounds (MULTI).  With `stack`, pm is a stack of maps (vhp_sweep_fronts_maps).
template <int R, bool MULTI, typename OutT>
hipError_t launch_sweep_t(vhp_ctx* c, const vhp::PackedMaps& pm, const int32_t* d_src, int n_src, OutT* d_out, const vhp::SweepPlan& plan,
                          const LaunchOpts& o, const vhp::MapStack* stack) {
  const int W = plan.W;
  const bool pack = c->opt_pack != 0;
  const size_t lds = vhp::sweep_lds_bytes(R, W, MULTI, pack);
  auto k = vhp::vhp_sweep_fronts<R, MULTI, OutT>;
  auto km = vhp::vhp_sweep_fronts_maps<R, MULTI, OutT>;
  {
    hipError_t e = raise_lds_limit(c, stack ? reinterpret_cast<const void*>(km) : reinterpret_cast<const void*>(k), lds);
    if (e != hipSuccess) return e;
  }
  vhp::DevMap m = dev_map(pm);
  const long long stride = o.field_stride > 0 ? o.field_stride : (long long)m.nx * m.ny;
  m.slide = plan.slide;
  hipError_t eb = vhp::attach_round_scratch(m, W * 64 * R, (size_t)n_src * vhp::kUnitsPerSource, c->d_bnd);
  if (eb != hipSuccess) return eb;
  const size_t n_units = (size_t)n_src * vhp::kUnitsPerSource;
  const int* order = nullptr;
  const int4* desc = nullptr;
  // per-launch timing: from before the unit-ordering pre-kernel (part of what a launch costs) to after the sweep
  EventPair ev;
  if (hipError_t ee = acquire_events(c, o.timed, &ev); ee != hipSuccess) return ee;
  if (ev.first) (void)hipEventRecord(ev.first, c->stream);
  if (n_src >= 8) {  // worth a 1-workgroup pre-kernel once the batch spans many CUs
    hipError_t eo = c->d_order.grow(n_units * (sizeof(int) + sizeof(int4)) + 16);
    if (eo != hipSuccess) { release_events(c, ev, eo); return eo; }
    int4* d_desc = reinterpret_cast<int4*>(c->d_order.get());  // n_units descriptors first (16-byte aligned)
    int* d_ord = reinterpret_cast<int*>(d_desc + n_units);     // then the order list
    // Packing short quadrants into one workgroup is implemented and parity-tested, but measured slower
    // on MI355X: off unless VHP_PACK is set.
    const int pack_w = (!MULTI && W == 8 && pack) ? W : 0;
    hipLaunchKernelGGL(vhp::vhp_order_units, dim3(1), dim3(1024), 0, c->stream, d_src, n_src, m.nx, m.ny, 64 * R, pack_w, d_ord,
                       d_desc);
    order = d_ord;
    desc = d_desc;
  }
  const unsigned grid = (unsigned)n_units;
  if (stack) hipLaunchKernelGGL(km, dim3(grid), dim3(128 * W), lds, c->stream, m, d_src, *stack, d_out, stride, c->d_err.get(), order, desc);
  else hipLaunchKernelGGL(k, dim3(grid), dim3(128 * W), lds, c->stream, m, d_src, d_out, stride, c->d_err.get(), order, desc);
  const hipError_t el = hipGetLastError();
  if (ev.first) (void)hipEventRecord(ev.second, c->stream);
  release_events(c, ev, el);
  return el;
}

// The pool sweep (lat = false) or the latency sweep (lat = true) on m, through vhp_batch_launch.h.  l: what a planner's loop adds to a
// latency sweep; with l.map_idx, m is the stack of maps and source s is swept on map l.map_idx[s] (its diagonal maps built: m.dmap).
template <typename OutT>
hipError_t launch_batch_sweep(vhp_ctx* c, const vhp::PackedMaps& m, const int32_t* d_src, int n_src, OutT* d_out, bool lat, const LaunchOpts& o,
                              const vhp::LatLaunch& l = {}) {
  // (the scratch is an allocation of its own: nothing but these two kernels may write the tagged lines)
  const size_t scratch = lat ? vhp::lat_scratch_bytes(n_src, m.nx, m.ny) : vhp::pool_scratch_bytes(n_src, m.nx, m.ny);
  if (c->d_pool.bytes() < scratch) {  // (zero when it is first used; the memset goes on the context's stream)
    hipError_t eo = c->d_pool.grow(scratch);
    if (eo == hipSuccess) eo = hipMemsetAsync(c->d_pool.get(), 0, scratch, c->stream);
    if (eo != hipSuccess) { c->d_pool.reset(); return eo; }
  }
  vhp::BatchArgs a;
  vhp::set_maps(a, m);
  a.d_src = d_src; a.n_src = n_src; a.d_out = d_out;
  a.dtype = sizeof(OutT) == 8 ? VHP_F64 : VHP_F32;
  a.field_stride = o.field_stride > 0 ? o.field_stride : (long long)m.nx * m.ny;
  a.d_err = c->d_err.get();
  a.d_queue = c->d_pool.get();
  a.pool_epoch = ++c->pool_epoch;
  a.lat = l;
  a.lat_workgroups = c->opt_lat_workgroups;
  if (lat)
    if (hipError_t eo = c->d_lat_order.grow(vhp::lat_order_bytes()); eo != hipSuccess) return eo;
  a.d_lat_order = c->d_lat_order.get();
  a.n_cus = c->n_cus;
  a.stream = c->stream;
  a.raise_lds = [c](const void* fn, size_t bytes) { return raise_lds_limit(c, fn, bytes); };
  a.pool = c->opt_pool;
  // timed by its own kernels' stamps in the slot the entry point took, tagged with the launch's epoch -- or by an event pair
  const bool stamped = o.stamp && o.stamp->stamped();
  if (stamped) {
    o.stamp->tag = a.pool_epoch;
    a.d_stamps = c->d_stamps.get() + c->ring.slot_offset(o.stamp->slot);
  }
  EventPair ev;
  if (hipError_t ee = acquire_events(c, o.timed && !stamped, &ev); ee != hipSuccess) return ee;
  a.ev_begin = ev.first;
  a.ev_end = ev.second;
  const hipError_t e = lat ? vhp::launch_lat(a) : vhp::launch_pool(a);
  release_events(c, ev, e);
  return e;
}

// The front sweep on pm in the build of plan p's shape.
template <typename OutT>
hipError_t launch_fronts(vhp_ctx* c, const vhp::PackedMaps& pm, const int32_t* d_src, int n_src, OutT* d_out, const vhp::SweepPlan& p,
                         const LaunchOpts& o, const vhp::MapStack* st = nullptr) {
  // (fp32 fields: only the one-row-per-lane builds exist, and the plan asks for no other)
  return vhp::with_sweep_shape(sizeof(OutT) == 4 ? 1 : p.R, p.multi, [&](auto r, auto mr) {
    if constexpr (sizeof(OutT) == 4 && r() != 1) return hipErrorInvalidValue;
    else return launch_sweep_t<r(), mr(), OutT>(c, pm, d_src, n_src, d_out, p, o, st);
  });
}

template <typename OutT>
hipError_t launch_sweep(vhp_ctx* c, const int32_t* d_src, int n_src, OutT* d_out, const LaunchOpts& o) {
  const vhp::SweepPlan p = plan_for(c, n_src, sizeof(OutT) == 8);
  c->last_kernel = p.kernel;
  if (p.kernel != 1) return launch_batch_sweep<OutT>(c, c->map, d_src, n_src, d_out, p.kernel == 4, o);
  return launch_fronts<OutT>(c, c->map, d_src, n_src, d_out, p, o);
}

// A batch on the stack of maps: always the front sweep (vhp_sweep_fronts_maps), in plan_for_maps's shape.
template <typename OutT>
hipError_t launch_maps_sweep(vhp_ctx* c, const int32_t* d_src, const int32_t* d_map_idx, int n_src, OutT* d_out, const LaunchOpts& o) {
  const vhp::SweepPlan p = plan_for_maps(c, n_src, sizeof(OutT) == 8);
  c->last_kernel = 1;
  const vhp::MapStack st = maps_stack(c->maps, d_map_idx);
  return launch_fronts<OutT>(c, c->maps, d_src, n_src, d_out, p, o, &st);
}

// What goes to the host through the context's scratch goes in slices of at most ~1 GiB: so many of n items of item_bytes each
int slice_items(int n, size_t item_bytes) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)1 << 30) / item_bytes)); }

// n items to out_host through the output scratch, slice by slice: produce(k0, nk, d) enqueues items k0 .. k0+nk-1 at d, then copy
// out, synchronise.  (The caller is on the context's device.)
template <typename Produce>
int copy_out_slices(vhp_ctx* ctx, const char* who, int n, size_t item_bytes, void* out_host, Produce produce) {
  const int slice = slice_items(n, item_bytes);
  const hipError_t e = ctx->d_out.grow((size_t)slice * item_bytes);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": scratch: " + hipGetErrorString(e));
  for (int k0 = 0; k0 < n; k0 += slice) {
    const int nk = std::min(slice, n - k0);
    if (const int rc = produce(k0, nk, ctx->d_out.get()); rc != VHP_OK) return rc;
    VHP_HIP(hipMemcpyAsync(static_cast<char*>(out_host) + (size_t)k0 * item_bytes, ctx->d_out.get(), (size_t)nk * item_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VHP_HIP(hipStreamSynchronize(ctx->stream));
  }
  return VHP_OK;
}

// The host-buffer sweeps' slices of fields of `field` bytes: a slice's sources copied to d_src, launch(s0, n) sweeps them -- sources
// s0 .. s0+n-1 -- into d_out.
template <typename Launch>
int stage_slices(vhp_ctx* ctx, const char* who, const int32_t* src_xy, int n_src, size_t field, void* out_host, Launch launch) {
  if (n_src == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  const hipError_t e = ctx->d_src.grow((size_t)slice_items(n_src, field) * 2 * sizeof(int32_t));
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": scratch: " + hipGetErrorString(e));
  return copy_out_slices(ctx, who, n_src, field, out_host, [&](int s0, int n, void*) -> int {
    VHP_HIP(hipMemcpyAsync(ctx->d_src.get(), src_xy + 2 * (size_t)s0, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return launch(s0, n);
  });
}

// ... of vhp_sweep_batch: the sources checked on the host first
template <typename Launch>
int stage_batch(vhp_ctx* ctx, const char* who, const int32_t* src_xy, int n_src, size_t esz, void* out_host, Launch launch) {
  for (int s = 0; s < n_src; ++s)
    if (src_xy[2 * s] < 0 || src_xy[2 * s + 1] < 0 || src_xy[2 * s] >= ctx->map.nx || src_xy[2 * s + 1] >= ctx->map.ny)
      return fail(ctx, VHP_ERR_SOURCE_OOB, "a sweep source lies outside the grid");
  return stage_slices(ctx, who, src_xy, n_src, (size_t)ctx->map.nx * ctx->map.ny * esz, out_host, [&](int, int n) { return launch(n); });
}

// ... on a stack: the slice's map indices, map_idx[s0 .. s0+n-1], at d_map_idx
int stage_map_idx(vhp_ctx* ctx, const char* who, const int32_t* map_idx, int s0, int n) {
  const hipError_t e = ctx->d_map_idx.grow((size_t)n * sizeof(int32_t));
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": scratch: " + hipGetErrorString(e));
  VHP_HIP(hipMemcpyAsync(ctx->d_map_idx.get(), map_idx + s0, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  return VHP_OK;
}

// ... and afterwards: a source the kernels rejected (vhp_raycast.hpp raycast_source_ok; map_idx null: the single map) leaves its field
// unwritten -- zero here, not what the scratch held
void zero_rejected_fields(const vhp::PackedMaps& m, const int32_t* src_xy, const int32_t* map_idx, int n_src, void* out_host, size_t field) {
  for (int i = 0; i < n_src; ++i)
    if (!vhp::raycast_source_ok(src_xy, map_idx, i, m.nx, m.ny, m.n)) std::memset(static_cast<char*>(out_host) + (size_t)i * field, 0, field);
}

int hip_rc(vhp_ctx* ctx, const char* what, hipError_t e) {
  return e == hipSuccess ? VHP_OK : fail(ctx, VHP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The device copy of the host array of `count` elements at src, in `staged` for this call only -- or src itself, already there
template <typename T>
int device_copy(vhp_ctx* ctx, const T* src, size_t count, bool from_device, vhp::DevBuf<T>& staged, const T** d) {
  *d = src;
  if (from_device) return VHP_OK;
  VHP_HIP(staged.grow(count * sizeof(T)));
  VHP_HIP(hipMemcpyAsync(staged.get(), src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  *d = staged.get();
  return VHP_OK;
}

// The single map from d_occ, with its diagonal maps where the latency sweep takes the grid.
int finish_set_map(vhp_ctx* ctx, int nx, int ny) {
  return hip_rc(ctx, "packing the map", vhp::maps_build(ctx->map, 1, nx, ny, ctx->stream, [&](vhp::PackedMaps& m) {
    hipError_t e = vhp::maps_pack(m, ctx->d_occ.get(), ctx->stream);
    if (e != hipSuccess || !vhp::lat_supported(nx, ny)) return e;
    const size_t bytes = vhp::lat_diag_map_bytes(nx, ny);
    e = m.dmap.grow(bytes);
    if (e == hipSuccess) e = hipMemsetAsync(m.dmap.get(), 0, bytes, ctx->stream);
    if (e == hipSuccess) e = vhp::lat_pack_diag_maps(ctx->d_occ.get(), nx, ny, m.dmap.get(), ctx->stream);
    return e;
  }));
}

// The single map replaced by the nx x ny map whose bytes fill(d_occ) enqueues: the stream drained, the old map and all that hangs on
// it dropped, then the new one whole -- or no map, not half of one.
template <typename Fill>
int replace_map(vhp_ctx* ctx, int nx, int ny, Fill fill) {
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  free_map(ctx);
  ctx->opt_field_stride = 0;  // (a stride belongs to a grid: one left over from a smaller grid would make the fields overlap)
  VHP_HIP(ctx->d_occ.grow((size_t)nx * ny));
  int rc = fill(ctx->d_occ.get());
  if (rc == VHP_OK) rc = finish_set_map(ctx, nx, ny);
  if (rc != VHP_OK) free_map(ctx);
  return rc;
}

// The stack of vhp_set_maps from the n_maps uint8 maps at src (host or device): both packed copies of every map, one launch each.
int build_maps(vhp_ctx* ctx, const uint8_t* src, int n_maps, int nx, int ny, bool from_device) {
  vhp::DevBuf<uint8_t> staged;
  const uint8_t* d_occ;
  if (const int rc = device_copy(ctx, src, (size_t)n_maps * nx * ny, from_device, staged, &d_occ); rc != VHP_OK) return rc;
  return hip_rc(ctx, "packing the maps", vhp::maps_build(ctx->maps, n_maps, nx, ny, ctx->stream, [&](vhp::PackedMaps& m) { return vhp::maps_pack(m, d_occ, ctx->stream); }));
}

// The stack of vhp_set_maps_windows: n_win windows of w x h of the single map, cut from its packed copies at the origins at src (host
// or device).
int build_windows(vhp_ctx* ctx, const int32_t* src, int n_win, int w, int h, bool from_device) {
  vhp::DevBuf<int32_t> staged;
  const int32_t* d_origin;
  if (const int rc = device_copy(ctx, src, (size_t)n_win * 2, from_device, staged, &d_origin); rc != VHP_OK) return rc;
  return hip_rc(ctx, "cutting the windows", vhp::maps_build(ctx->maps, n_win, w, h, ctx->stream, [&](vhp::PackedMaps& m) { return vhp::maps_cut(m, ctx->map, d_origin, ctx->stream); }));
}

// The footprint of vhp_inflate_map / vhp_inflate_maps, or why not
int inflate_footprint(vhp_ctx* ctx, const char* who, int shape, int p, int flags, vhp::InflateTable* t) {
  static_assert(vhp::kMaxInflate == VHP_MAX_INFLATE, "vhp_inflate.hpp and vhp.h disagree on the largest reach");
  if ((flags & ~VHP_INFLATE_BORDER) != 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": unknown flag");
  if (!vhp::inflate_table(shape, p, t)) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": unknown shape, p < 0 or a reach above VHP_MAX_INFLATE");
  return VHP_OK;
}

// G of a batch solve (vhp_planner_solve_batch): the largest of 32, 16, 8, 4, 2 for which a launch of G sources takes the latency sweep
// and G queries' state fits in a quarter of the free device memory, else 1 -- capped by "planner_batch_group" --; 0 where even one
// source does not take the latency sweep (the queries then run one by one on the front sweep).
// (On the stack of maps: the same rule on the stack's nx x ny.)
int planner_batch_group_size(const vhp_ctx* c, const vhp::PackedMaps& m, uint64_t max_iter) {
  if (plan_for_grid(c, m, 1, true).kernel != 4) return 0;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
  const size_t per_query = vhp::kBatchBytesPerCell * (size_t)m.nx * m.ny + 2 * (size_t)(max_iter + 2) * sizeof(int32_t);
  int g = 1;
  for (int G = vhp::kBatchMaxGroup; G > 1; G /= 2)
    if (plan_for_grid(c, m, G, true).kernel == 4 && (size_t)G * per_query <= free_b / 4) { g = G; break; }
  return c->opt_planner_batch_group > 0 ? std::min(g, c->opt_planner_batch_group) : g;
}

// The batch planner's state on the single map, or with `maps` on the stack: its queries, its maps, and what a call that finds no
// solved batch there says after its name.
struct BatchOn {
  vhp::BatchState& b;
  vhp::PackedMaps& m;
  const char* none_solved;
};
BatchOn batch_on(vhp_ctx* ctx, bool maps) {
  if (maps) return {ctx->maps_batch, ctx->maps, ": no maps batch solved on this stack"};
  return {ctx->batch, ctx->map, ": no batch solved on this map"};
}

// The last batch's slot of query q, or an error for the _results entry points.
int batch_slot(vhp_ctx* ctx, const char* who, bool maps, int q, int* slot) {
  const auto [b, m, none_solved] = batch_on(ctx, maps);
  if (!b.solved) return fail(ctx, VHP_ERR_ARG, std::string(who) + none_solved);
  if (q < 0 || q >= (int)b.slot_of.size()) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": query index out of range");
  if (b.slot_of[q] < 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": query " + std::to_string(q) + " failed validation and has no results");
  *slot = b.slot_of[q];
  return VHP_OK;
}

// A plain or speculative solve that returned before it ran (one of the four validation codes, or VHP_ERR_ARG): vhp_planner_path
// reports that code for its query.
void note_unsolved(vhp_ctx* ctx, int rc) {
  if (rc == VHP_ERR_ARG || (rc >= VHP_ERR_START_OOB && rc <= VHP_ERR_END_OCCUPIED)) {
    ctx->pl.path_state = 2;
    ctx->pl.last_code = rc;
  }
}

// What vhp_planner_solve and vhp_planner_solve_speculative do around their solve: the checks before it, the plan of its sweeps (n_src
// sources per launch, n_workgroups of round scratch for the front sweep), and what the context keeps of how it ended.  solve(pm, plan,
// &msg) sets the latency launches the plan allows on ctx->pl and runs the solve.
template <typename Solve>
int planner_call(vhp_ctx* ctx, const char* who, int n_src, size_t n_workgroups, Solve solve) {
  if (!ctx) return VHP_ERR_ARG;
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, std::string(who) + ": no map set");
  VHP_ON_DEVICE(ctx);
  std::string msg;
  vhp::DevMap pm = dev_map(ctx->map);
  vhp::SweepPlan plan;
  hipError_t eb = plan_planner(ctx, pm, n_src, n_workgroups, &plan);
  if (eb != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("scratch: ") + hipGetErrorString(eb));
  ctx->pl.path_state = 0;
  const int rc = solve(pm, plan, &msg);
  note_unsolved(ctx, rc);
  ctx->timed.events();
  if (rc != VHP_OK) ctx->err = msg;
  return rc;
}

// What a path call reads of the last batch on b (nx x ny): every query's slot or validation code, its n_pivots, the slots' arrays.
vhp::PathsDev batch_paths_dev(const vhp::BatchState& b, const std::vector<int32_t>& codes, int nx, int ny) {
  vhp::PathsDev p{};
  p.label = b.label.get();
  p.pivots = b.pivots.get();
  p.label_stride = b.cells;
  p.pivot_stride = b.pivot_stride;
  p.query = b.query.get();
  p.nx = nx;
  p.ny = ny;
  p.n_queries = (int)b.slot_of.size();
  for (int q = 0; q < p.n_queries; ++q) {
    const int k = b.slot_of[q];
    p.slot[q] = (int16_t)(k >= 0 ? k : -codes[q]);
    p.nb[q] = k >= 0 ? (uint32_t)b.h_ctl[k].ctl.nb : 0u;
  }
  return p;
}

// The last plain / speculative solve as a batch of one.
vhp::PathsDev plain_paths_dev(const vhp_ctx* ctx) {
  const vhp::PlannerState& s = ctx->pl;
  vhp::PathsDev p{};
  p.label = s.label.get();
  p.pivots = s.pivots.get();
  p.query = nullptr;
  p.end_x = s.last_end_x;
  p.end_y = s.last_end_y;
  p.nx = ctx->map.nx;
  p.ny = ctx->map.ny;
  p.n_queries = 1;
  p.slot[0] = (int16_t)(s.path_state == 1 ? 0 : -s.last_code);
  p.nb[0] = s.path_state == 1 ? s.last_nb : 0u;
  return p;
}

// The six path entry points behind one body: the device form launches into the caller's buffers, the host form through staging.
int paths_call(vhp_ctx* ctx, const char* who, vhp::PathsDev p, bool device, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length,
               int32_t* path_status) {
  VHP_ON_DEVICE(ctx);
  hipError_t e;
  if (device) {
    p.path_xy = path_xy;
    p.cap = cap;
    p.n_path = n_path;
    p.length = length;
    p.status = path_status;
    e = vhp::paths_launch(ctx->paths, p, ctx->stream);
  } else {
    e = vhp::paths_host(ctx->paths, p, ctx->stream, path_xy, cap, n_path, length, path_status);
  }
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return VHP_OK;
}

int batch_paths(vhp_ctx* ctx, const char* who, bool maps, bool device, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length,
                int32_t* path_status) {
  if (!ctx) return VHP_ERR_ARG;
  const auto [b, m, none_solved] = batch_on(ctx, maps);
  if (!b.solved) return fail(ctx, VHP_ERR_ARG, std::string(who) + none_solved);
  return paths_call(ctx, who, batch_paths_dev(b, b.codes, m.nx, m.ny), device, path_xy, cap, n_path, length, path_status);
}

int plain_path(vhp_ctx* ctx, const char* who, bool device, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status) {
  if (!ctx) return VHP_ERR_ARG;
  if (ctx->pl.path_state == 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": no planner solve has run on this map");
  return paths_call(ctx, who, plain_paths_dev(ctx), device, path_xy, cap, n_path, length, path_status);
}

// The solve a tree call names (vhp_solve_kind), as the path calls see it: the last plain / speculative solve as a batch of one, the
// last batch, the last maps batch.  The errors are those of the path calls.
int tree_solve(vhp_ctx* ctx, const char* who, int solve, vhp::PathsDev* p) {
  if (solve == VHP_SOLVE_PLAIN) {
    if (ctx->pl.path_state == 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": no planner solve has run on this map");
    *p = plain_paths_dev(ctx);
    return VHP_OK;
  }
  if (solve != VHP_SOLVE_BATCH && solve != VHP_SOLVE_MAPS_BATCH) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": solve is not a vhp_solve_kind");
  const auto [b, m, none_solved] = batch_on(ctx, solve == VHP_SOLVE_MAPS_BATCH);
  if (!b.solved) return fail(ctx, VHP_ERR_ARG, std::string(who) + none_solved);
  *p = batch_paths_dev(b, b.codes, m.nx, m.ny);
  return VHP_OK;
}

int length_fields(vhp_ctx* ctx, const char* who, bool device, int solve, int q_first, int n_q, double* length, uint32_t* n_path) {
  if (!ctx) return VHP_ERR_ARG;
  vhp::PathsDev p{};
  if (int rc = tree_solve(ctx, who, solve, &p); rc != VHP_OK) return rc;
  if (q_first < 0 || n_q < 1 || q_first > p.n_queries - n_q) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": query range outside the solve's queries");
  if (!length && !n_path) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": both outputs are null");
  if (device && ((reinterpret_cast<uintptr_t>(length) & 7) || (reinterpret_cast<uintptr_t>(n_path) & 3)))
    return fail(ctx, VHP_ERR_ARG, std::string(who) + ": an output is not aligned to its element type");
  VHP_ON_DEVICE(ctx);
  const hipError_t e = device ? vhp::tree_fields_launch(ctx->tree, p, q_first, n_q, ctx->stream, length, n_path)
                              : vhp::tree_fields_host(ctx->tree, p, q_first, n_q, ctx->stream, length, n_path);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return VHP_OK;
}

int goal_paths(vhp_ctx* ctx, const char* who, bool device, int solve, const int32_t* goals, int n_goals, int32_t* path_xy, uint32_t cap,
               uint32_t* n_path, double* length, int32_t* path_status) {
  if (!ctx) return VHP_ERR_ARG;
  vhp::PathsDev p{};
  if (int rc = tree_solve(ctx, who, solve, &p); rc != VHP_OK) return rc;
  if (n_goals < 0 || (n_goals > 0 && !goals)) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": null goals or a negative count");
  if (n_goals == 0) return VHP_OK;
  if (device && ((reinterpret_cast<uintptr_t>(length) & 7) || ((reinterpret_cast<uintptr_t>(goals) | reinterpret_cast<uintptr_t>(path_xy) |
                                                                 reinterpret_cast<uintptr_t>(n_path) | reinterpret_cast<uintptr_t>(path_status)) & 3)))
    return fail(ctx, VHP_ERR_ARG, std::string(who) + ": a buffer is not aligned to its element type");
  if (!device)
    for (int g = 0; g < n_goals; ++g)
      if (goals[3 * (size_t)g] < 0 || goals[3 * (size_t)g] >= p.n_queries)
        return fail(ctx, VHP_ERR_ARG, std::string(who) + ": goal " + std::to_string(g) + " names a query outside the solve's queries");
  VHP_ON_DEVICE(ctx);
  hipError_t e;
  if (device) {
    vhp::TreeGoalArgs a{};
    a.goals = goals;
    a.n_goals = n_goals;
    a.path_xy = path_xy;
    a.cap = cap;
    a.n_path = n_path;
    a.length = length;
    a.status = path_status;
    e = vhp::tree_goals_launch(ctx->tree, p, ctx->stream, a);
  } else {
    e = vhp::tree_goals_host(ctx->tree, p, ctx->stream, goals, n_goals, path_xy, cap, n_path, length, path_status);
  }
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return VHP_OK;
}

// ---- ray casting for batches of sources (vhp_raycast.hip): what the entry points below share
size_t raycast_elem_bytes(int dtype) { return dtype == VHP_F64 ? 8 : dtype == VHP_F32 ? 4 : dtype == VHP_U8 ? 1 : 0; }

vhp::PackedOcc packed_occ(const vhp::PackedMaps& p) { return {p.rows.get(), p.cols.get(), p.wpr, p.wpc}; }

// The device form on the single map (d_map_idx null) or on the stack: packed fields, timed as vhp_raycast_all is (fill plus kernel).
int raycast_device(vhp_ctx* ctx, const char* who, bool maps, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out) {
  if (!ctx || !d_src_xy || !d_out || n_src < 0 || (maps && !d_map_idx)) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad argument");
  const vhp::PackedMaps& m = maps ? ctx->maps : ctx->map;
  if (!m.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, std::string(who) + (maps ? ": no maps set" : ": no map set"));
  const size_t esz = raycast_elem_bytes(dtype);
  if (!esz) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  if (reinterpret_cast<uintptr_t>(d_out) % esz != 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": d_out is not aligned to its element type");
  if (n_src == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  vhp::RaycastLaunch l;
  l.d_out = d_out;
  l.dtype = dtype;
  l.d_src_xy = d_src_xy;
  l.n_src = n_src;
  l.nx = m.nx;
  l.ny = m.ny;
  l.occ = packed_occ(m);
  l.d_map_idx = d_map_idx;
  l.n_maps = m.n;
  l.rows_stride = vhp::map_rows(m, 1) - vhp::map_rows(m, 0);
  l.cols_stride = vhp::map_cols(m, 1) - vhp::map_cols(m, 0);
  l.d_err = ctx->d_err.get();
  l.stream = ctx->stream;
  const hipError_t e = vhp::launch_raycast(l);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed.events();
  return VHP_OK;
}

// The host form: slices through the context's scratch like the sweeps; a source that is not cast leaves its field 0.
int raycast_host(vhp_ctx* ctx, const char* who, bool maps, const int32_t* src_xy, const int32_t* map_idx, int n_src, int dtype, void* out_host) {
  if (!ctx || !src_xy || !out_host || n_src < 0 || (maps && !map_idx)) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad argument");
  const vhp::PackedMaps& m = maps ? ctx->maps : ctx->map;
  if (!m.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, std::string(who) + (maps ? ": no maps set" : ": no map set"));
  const size_t esz = raycast_elem_bytes(dtype);
  if (!esz) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  const size_t field = (size_t)m.nx * m.ny * esz;
  int rc = stage_slices(ctx, who, src_xy, n_src, field, out_host, [&](int s0, int n) -> int {
    if (maps)
      if (const int r = stage_map_idx(ctx, who, map_idx, s0, n); r != VHP_OK) return r;
    return raycast_device(ctx, who, maps, ctx->d_src.get(), maps ? ctx->d_map_idx.get() : nullptr, n, dtype, ctx->d_out.get());
  });
  if (rc != VHP_OK || n_src == 0) return rc;
  rc = vhp_sync(ctx);
  zero_rejected_fields(m, src_xy, maps ? map_idx : nullptr, n_src, out_host, field);
  return rc;
}

}  // namespace

extern "C" {

const char* vhp_version(void) { return "vhp-hip 0.1 gfx950"; }

int vhp_create(int device_ordinal, vhp_ctx** out) {
  if (!out) return VHP_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VHP_ERR_HIP;
  if (device_ordinal < 0 || device_ordinal >= n) return VHP_ERR_ARG;
  vhp_ctx* ctx = new vhp_ctx();
  ctx->device = device_ordinal;
  DeviceGuard guard(device_ordinal);
  if (!guard.ok || hipStreamCreate(&ctx->own_stream) != hipSuccess ||
      create_timing_event(&ctx->ev0) != hipSuccess || create_timing_event(&ctx->ev1) != hipSuccess ||
      ctx->d_err.grow(sizeof(int)) != hipSuccess || hipMemset(ctx->d_err.get(), 0, sizeof(int)) != hipSuccess) {
    delete ctx;  // (on its device: the guard is still in scope)
    return VHP_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cus = prop.multiProcessorCount;
  }
  // the stamps' clock and slot 0 (the launches with vhp_timing off); a slot holds a launch of up to one workgroup per CU.  Without the
  // clock's rate, or without the memory, no launch is stamped: the events time them all.
  if (VHP_TIMING_STAMPS) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_ordinal) == hipSuccess && khz > 0) ctx->clock_khz = khz;
    else (void)hipGetLastError();
    ctx->ring.resize(0, ctx->n_cus);
    if (ctx->clock_khz > 0 && allocate_stamps(ctx) != hipSuccess) (void)hipGetLastError();
  }
  *out = ctx;
  return VHP_OK;
}

int vhp_destroy(vhp_ctx* ctx) {
  if (!ctx) return VHP_ERR_ARG;
  DeviceGuard guard(ctx->device);
  hipStreamSynchronize(ctx->stream);
  free_map(ctx);
  free_maps(ctx);
  for (auto& t : ctx->timed_launches)
    if (t.ev.first) { (void)hipEventDestroy(t.ev.first); (void)hipEventDestroy(t.ev.second); }
  for (auto& pr : ctx->event_pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (void* p : ctx->placed) (void)hipFree(p);
  if (ctx->ev0) hipEventDestroy(ctx->ev0);
  if (ctx->ev1) hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
  delete ctx;  // (its buffers go here, on the context's device: the guard is still in scope)
  return VHP_OK;
}

const char* vhp_last_error(const vhp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vhp_set_stream(vhp_ctx* ctx, void* hip_stream) {
  if (!ctx) return VHP_ERR_ARG;
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return VHP_OK;
}

static int set_map_common(vhp_ctx* ctx, const uint8_t* src, int nx, int ny, bool from_device) {
  if (!ctx || !src || nx <= 0 || ny <= 0) return fail(ctx, VHP_ERR_ARG, "vhp_set_map: bad argument");
  if (nx > VHP_MAX_SIDE || ny > VHP_MAX_SIDE) return fail(ctx, VHP_ERR_TOO_LARGE, "vhp_set_map: grid side exceeds VHP_MAX_SIDE");
  VHP_ON_DEVICE(ctx);
  const size_t n = (size_t)nx * ny;
  const int rc = replace_map(ctx, nx, ny, [&](uint8_t* d_occ) -> int {
    VHP_HIP(hipMemcpyAsync(d_occ, src, n, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return VHP_OK;
  });
  if (rc != VHP_OK) return rc;  // (nothing half-set: neither the old grid's sides with the new grid's arrays nor a host copy of a map that is not there)
  if (!from_device) ctx->h_occ.assign(src, src + n);
  ctx->pl.h_occ = ctx->h_occ.empty() ? nullptr : ctx->h_occ.data();
  return VHP_OK;
}

int vhp_set_map(vhp_ctx* ctx, const uint8_t* occ, int nx, int ny) { return set_map_common(ctx, occ, nx, ny, false); }
int vhp_set_map_device(vhp_ctx* ctx, const uint8_t* d_occ, int nx, int ny) { return set_map_common(ctx, d_occ, nx, ny, true); }

// vhp_sweep_batch_device writing its fields o.field_stride apart (the entry point: the option; the host-buffer form: packed)
static int sweep_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, int n_src, int variant, int dtype, void* d_out, const LaunchOpts& o) {
  if (!ctx || !d_src_xy || !d_out || n_src < 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_device: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_batch_device: no map set");
  if (dtype != VHP_F64 && dtype != VHP_F32) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  if (variant != VHP_SWEEP_FULL && variant != VHP_SWEEP_QUEUE) return fail(ctx, VHP_ERR_ARG, "bad variant");
  // (any alignment of whole elements is swept -- the kernels' builds for fields off the 16-byte grid --, a pointer inside an element is not)
  if (reinterpret_cast<uintptr_t>(d_out) % (dtype == VHP_F64 ? 8 : 4) != 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_device: d_out is not aligned to its element type");
  if (o.field_stride > 0 && o.field_stride < (long long)ctx->map.nx * ctx->map.ny)
    return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_device: field_stride is smaller than a field (nx * ny elements): the fields would overlap");
  if (variant == VHP_SWEEP_QUEUE && o.field_stride > 0 && o.field_stride != (long long)ctx->map.nx * ctx->map.ny)
    return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_device: the queue variant writes packed fields (field_stride must be 0)");
  if (n_src == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  // A pool- or latency-sweep launch times itself by the stamps its kernels write, and nothing is recorded on the stream for it; every
  // other launch -- and one of those two that has no slot for its stamps -- between ev0 and ev1 (and vhp_timing's pair inside).
  vhp::stamps::Launch st = take_stamp_slot(ctx, variant == VHP_SWEEP_QUEUE ? 0 : plan_for(ctx, n_src, dtype == VHP_F64).kernel, n_src, o.timed);
  LaunchOpts lo = o;
  lo.stamp = &st;
  const bool ring_slot = st.slot > 0;
  if (!st.stamped()) {
    // (ev0 moves before the launch is known to go out: from here on the old pair says nothing, whatever happens below)
    if (ctx->timed.state == vhp::stamps::Last::kEvents) ctx->timed.nothing();
    VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  }
  hipError_t e;
  if (variant == VHP_SWEEP_QUEUE) {
    e = vhp::launch_queue_sweep_impl(ctx->qs, dev_map(ctx->map), ctx->d_occ.get(), d_src_xy, n_src, dtype, d_out, ctx->d_err.get(), ctx->stream);
  } else if (dtype == VHP_F64) {
    e = launch_sweep<double>(ctx, d_src_xy, n_src, static_cast<double*>(d_out), lo);
  } else {
    e = launch_sweep<float>(ctx, d_src_xy, n_src, static_cast<float*>(d_out), lo);
  }
  if (e != hipSuccess) {  // (its slot back to the ring; what vhp_last_elapsed_ms reports stays what it was)
    if (ring_slot) ctx->ring.untake();
    return fail(ctx, VHP_ERR_HIP, std::string("sweep launch: ") + hipGetErrorString(e));
  }
  if (st.stamped()) {
    if (ring_slot) ctx->timed_launches.push_back({{nullptr, nullptr}, st});
    ctx->timed.stamps(st);
    return VHP_OK;
  }
  VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed.events();
  return VHP_OK;
}

int vhp_sweep_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, int n_src, int variant, int dtype, void* d_out) {
  return sweep_batch_device(ctx, d_src_xy, n_src, variant, dtype, d_out, {ctx ? ctx->opt_field_stride : 0, ctx && ctx->timing});
}

int vhp_sync(vhp_ctx* ctx) {
  if (!ctx) return VHP_ERR_ARG;
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  int flag = 0;
  VHP_HIP(hipMemcpy(&flag, ctx->d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (flag) {
    VHP_HIP(hipMemset(ctx->d_err.get(), 0, sizeof(int)));
    return fail(ctx, VHP_ERR_SOURCE_OOB, "a sweep source lies outside the grid");
  }
  return VHP_OK;
}

int vhp_sweep_batch(vhp_ctx* ctx, const int32_t* src_xy, int n_src, int variant, int dtype, void* out_host) {
  if (!ctx || !src_xy || !out_host || n_src < 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_batch: no map set");
  if (dtype != VHP_F64 && dtype != VHP_F32) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  // (the library's own scratch holds packed fields and is copied out packed: "field_stride" is a property of a caller's device buffer)
  const int rc = stage_batch(ctx, "vhp_sweep_batch", src_xy, n_src, dtype == VHP_F64 ? 8 : 4, out_host,
                             [&](int n) { return sweep_batch_device(ctx, ctx->d_src.get(), n, variant, dtype, ctx->d_out.get(), {0, ctx->timing}); });
  return rc == VHP_OK && n_src > 0 ? vhp_sync(ctx) : rc;
}

static int set_maps_common(vhp_ctx* ctx, const uint8_t* src, int n_maps, int nx, int ny, bool from_device) {
  const std::string who = from_device ? "vhp_set_maps_device" : "vhp_set_maps";
  if (!ctx || !src || n_maps < 1 || nx <= 0 || ny <= 0) return fail(ctx, VHP_ERR_ARG, who + ": bad argument");
  if (nx > VHP_MAX_SIDE || ny > VHP_MAX_SIDE) return fail(ctx, VHP_ERR_TOO_LARGE, who + ": grid side exceeds VHP_MAX_SIDE");
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  free_maps(ctx);  // ("field_stride" stays: vhp_set_map owns its reset)
  const int rc = build_maps(ctx, src, n_maps, nx, ny, from_device);
  if (rc != VHP_OK) free_maps(ctx);  // (an empty stack, not a half-built one)
  return rc;
}

int vhp_set_maps(vhp_ctx* ctx, const uint8_t* occ, int n_maps, int nx, int ny) { return set_maps_common(ctx, occ, n_maps, nx, ny, false); }
int vhp_set_maps_device(vhp_ctx* ctx, const uint8_t* d_occ, int n_maps, int nx, int ny) { return set_maps_common(ctx, d_occ, n_maps, nx, ny, true); }

static int set_maps_windows_common(vhp_ctx* ctx, const int32_t* origin_xy, int n_windows, int w, int h, bool from_device) {
  const std::string who = from_device ? "vhp_set_maps_windows_device" : "vhp_set_maps_windows";
  if (!ctx || !origin_xy || n_windows < 1 || w <= 0 || h <= 0) return fail(ctx, VHP_ERR_ARG, who + ": bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, who + ": no map set");
  if (w > VHP_MAX_SIDE || h > VHP_MAX_SIDE) return fail(ctx, VHP_ERR_TOO_LARGE, who + ": window side exceeds VHP_MAX_SIDE");
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  free_maps(ctx);  // (as vhp_set_maps: the single map, the planner's state and "field_stride" stay)
  const int rc = build_windows(ctx, origin_xy, n_windows, w, h, from_device);
  if (rc != VHP_OK) free_maps(ctx);
  return rc;
}

int vhp_set_maps_windows(vhp_ctx* ctx, const int32_t* origin_xy, int n_windows, int w, int h) {
  return set_maps_windows_common(ctx, origin_xy, n_windows, w, h, false);
}
int vhp_set_maps_windows_device(vhp_ctx* ctx, const int32_t* d_origin_xy, int n_windows, int w, int h) {
  return set_maps_windows_common(ctx, d_origin_xy, n_windows, w, h, true);
}

// The packed maps a call reads -- `single`: the map of vhp_set_map, a stack of one; else the stack of vhp_set_maps -- and its maps
// first .. first+n-1, checked to lie in them.
static int select_maps(vhp_ctx* ctx, const char* who, bool single, int first, int n, vhp::PackedMaps** m) {
  *m = single ? &ctx->map : &ctx->maps;
  if (!(*m)->rows.get()) return fail(ctx, VHP_ERR_NO_MAP, std::string(who) + (single ? ": no map set" : ": no maps set"));
  if (n < 1 || first < 0 || first >= (*m)->n || n > (*m)->n - first) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": maps outside the stack");
  return VHP_OK;
}

// The four occupancy calls: the maps' bytes at `out`, on the device or on the host through the scratch
static int occupancy(vhp_ctx* ctx, const char* who, bool single, int first, int n, uint8_t* out, bool device) {
  if (!ctx || !out || n < 1) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad argument");
  vhp::PackedMaps* m;
  if (const int rc = select_maps(ctx, who, single, first, n, &m); rc != VHP_OK) return rc;
  VHP_ON_DEVICE(ctx);
  auto unpack = [&](int k0, int nk, void* d) { return hip_rc(ctx, who, vhp::maps_unpack(*m, first + k0, nk, static_cast<uint8_t*>(d), ctx->stream)); };
  return device ? unpack(0, n, out) : copy_out_slices(ctx, who, n, (size_t)m->nx * m->ny, out, unpack);
}

int vhp_maps_occupancy_device(vhp_ctx* ctx, int first, int n, uint8_t* d_occ_out) {
  return occupancy(ctx, "vhp_maps_occupancy_device", false, first, n, d_occ_out, true);
}
int vhp_maps_occupancy(vhp_ctx* ctx, int first, int n, uint8_t* occ_out) { return occupancy(ctx, "vhp_maps_occupancy", false, first, n, occ_out, false); }
int vhp_map_occupancy_device(vhp_ctx* ctx, uint8_t* d_occ_out) { return occupancy(ctx, "vhp_map_occupancy_device", true, 0, 1, d_occ_out, true); }
int vhp_map_occupancy(vhp_ctx* ctx, uint8_t* occ_out) { return occupancy(ctx, "vhp_map_occupancy", true, 0, 1, occ_out, false); }

int vhp_inflate_map(vhp_ctx* ctx, int shape, int p, int flags) {
  if (!ctx) return VHP_ERR_ARG;
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_inflate_map: no map set");
  vhp::InflateTable t;
  if (const int rc = inflate_footprint(ctx, "vhp_inflate_map", shape, p, flags, &t); rc != VHP_OK) return rc;
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  // the inflated rows into scratch (their data words: all the unpacking reads) while the old map is there, then the new map from their bytes
  const int nx = ctx->map.nx, ny = ctx->map.ny, wpr = ctx->map.wpr;
  VHP_HIP(ctx->d_inflate.grow((size_t)ny * wpr * 8));
  VHP_HIP(vhp::maps_inflate_copy(ctx->map.rows.get(), ctx->d_inflate.get(), 1, ny, nx, wpr, t, flags & VHP_INFLATE_BORDER, ctx->stream));
  return replace_map(ctx, nx, ny, [&](uint8_t* d_occ) {
    return hip_rc(ctx, "vhp_inflate_map: unpack", vhp::maps_unpack(ctx->d_inflate.get(), 1, nx, ny, wpr, d_occ, ctx->stream));
  });
}

int vhp_inflate_maps(vhp_ctx* ctx, int first, int n, int shape, int p, int flags) {
  if (!ctx) return VHP_ERR_ARG;
  vhp::PackedMaps* pm;
  if (const int rc = select_maps(ctx, "vhp_inflate_maps", false, first, n, &pm); rc != VHP_OK) return rc;
  vhp::PackedMaps& m = *pm;
  vhp::InflateTable t;
  if (const int rc = inflate_footprint(ctx, "vhp_inflate_maps", shape, p, flags, &t); rc != VHP_OK) return rc;
  VHP_ON_DEVICE(ctx);
  // both copies of the range into scratch -- zeroed first: the pads --, then over the range; anything that fails empties the stack
  const size_t row_words = (size_t)n * m.ny * m.wpr, col_words = (size_t)n * m.nx * m.wpc;
  uint64_t* const rows = vhp::map_rows(m, first);
  uint64_t* const cols = vhp::map_cols(m, first);
  const int border = flags & VHP_INFLATE_BORDER;
  const int rc = [&]() -> int {
    VHP_HIP(hipStreamSynchronize(ctx->stream));
    VHP_HIP(ctx->d_inflate.grow((row_words + col_words) * 8));
    uint64_t* const new_rows = ctx->d_inflate.get();
    uint64_t* const new_cols = new_rows + row_words;
    VHP_HIP(hipMemsetAsync(new_rows, 0, (row_words + col_words) * 8, ctx->stream));
    VHP_HIP(vhp::maps_inflate_copy(rows, new_rows, n, m.ny, m.nx, m.wpr, t, border, ctx->stream));
    VHP_HIP(vhp::maps_inflate_copy(cols, new_cols, n, m.nx, m.ny, m.wpc, t, border, ctx->stream));
    VHP_HIP(hipMemcpyAsync(rows, new_rows, row_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    VHP_HIP(hipMemcpyAsync(cols, new_cols, col_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    VHP_HIP(hipStreamSynchronize(ctx->stream));
    return VHP_OK;
  }();
  if (rc != VHP_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    free_maps(ctx);
    return rc;
  }
  m.dmap.reset();  // (built again by the next planner batch on the stack that takes the latency sweep)
  vhp::batch_free(ctx->maps_batch);
  return VHP_OK;
}

// The four clearance calls.  The checks in the order of the header: the pointer, the map or stack, the range, the flags and the
// footprint, and for the device forms the pointer's alignment.  The host forms go through the scratch (one slice, and one launch, for
// anything under ~1 GiB of field).
static int clearance(vhp_ctx* ctx, const char* who, bool single, int first, int n, int shape, int p_max, int flags, uint16_t* out, bool device) {
  static_assert(vhp::kClearanceFar == VHP_CLEARANCE_FAR, "vhp_clearance.hpp and vhp.h disagree on the far value");
  if (!ctx || !out) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad argument");
  vhp::PackedMaps* m;
  if (const int rc = select_maps(ctx, who, single, first, n, &m); rc != VHP_OK) return rc;
  vhp::InflateTable t;
  if (const int rc = inflate_footprint(ctx, who, shape, p_max, flags, &t); rc != VHP_OK) return rc;
  if (device && (reinterpret_cast<uintptr_t>(out) & 1) != 0) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": d_out is not aligned to 2 bytes");
  VHP_ON_DEVICE(ctx);
  auto launch = [&](int k0, int nk, void* d) {
    return hip_rc(ctx, who, vhp::maps_clearance(*m, first + k0, nk, shape, p_max, t.reach, flags & VHP_INFLATE_BORDER, static_cast<uint16_t*>(d), ctx->stream));
  };
  return device ? launch(0, n, out) : copy_out_slices(ctx, who, n, (size_t)m->nx * m->ny * 2, out, launch);
}

int vhp_map_clearance(vhp_ctx* ctx, int shape, int p_max, int flags, uint16_t* out) {
  return clearance(ctx, "vhp_map_clearance", true, 0, 1, shape, p_max, flags, out, false);
}
int vhp_map_clearance_device(vhp_ctx* ctx, int shape, int p_max, int flags, uint16_t* d_out) {
  return clearance(ctx, "vhp_map_clearance_device", true, 0, 1, shape, p_max, flags, d_out, true);
}
int vhp_maps_clearance(vhp_ctx* ctx, int first, int n, int shape, int p_max, int flags, uint16_t* out) {
  return clearance(ctx, "vhp_maps_clearance", false, first, n, shape, p_max, flags, out, false);
}
int vhp_maps_clearance_device(vhp_ctx* ctx, int first, int n, int shape, int p_max, int flags, uint16_t* d_out) {
  return clearance(ctx, "vhp_maps_clearance_device", false, first, n, shape, p_max, flags, d_out, true);
}

static int sweep_maps_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out,
                                   const LaunchOpts& o) {
  if (!ctx || !d_src_xy || !d_map_idx || !d_out || n_src < 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_maps_batch_device: bad argument");
  if (!ctx->maps.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_maps_batch_device: no maps set");
  if (dtype != VHP_F64 && dtype != VHP_F32) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  if (reinterpret_cast<uintptr_t>(d_out) % (dtype == VHP_F64 ? 8 : 4) != 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_maps_batch_device: d_out is not aligned to its element type");
  if (o.field_stride > 0 && o.field_stride < (long long)ctx->maps.nx * ctx->maps.ny)
    return fail(ctx, VHP_ERR_ARG, "vhp_sweep_maps_batch_device: field_stride is smaller than a field (nx * ny elements): the fields would overlap");
  if (n_src == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  const hipError_t e = dtype == VHP_F64 ? launch_maps_sweep<double>(ctx, d_src_xy, d_map_idx, n_src, static_cast<double*>(d_out), o)
                                        : launch_maps_sweep<float>(ctx, d_src_xy, d_map_idx, n_src, static_cast<float*>(d_out), o);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("maps sweep launch: ") + hipGetErrorString(e));
  VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed.events();
  return VHP_OK;
}

int vhp_sweep_maps_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out) {
  return sweep_maps_batch_device(ctx, d_src_xy, d_map_idx, n_src, dtype, d_out, {ctx ? ctx->opt_field_stride : 0, ctx && ctx->timing});
}

int vhp_sweep_maps_batch(vhp_ctx* ctx, const int32_t* src_xy, const int32_t* map_idx, int n_src, int dtype, void* out_host) {
  if (!ctx || !src_xy || !map_idx || !out_host || n_src < 0) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_maps_batch: bad argument");
  if (!ctx->maps.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_maps_batch: no maps set");
  if (dtype != VHP_F64 && dtype != VHP_F32) return fail(ctx, VHP_ERR_ARG, "bad dtype");
  const size_t field = (size_t)ctx->maps.nx * ctx->maps.ny * (dtype == VHP_F64 ? 8 : 4);
  int rc = stage_slices(ctx, "vhp_sweep_maps_batch", src_xy, n_src, field, out_host, [&](int s0, int n) -> int {
    if (const int r = stage_map_idx(ctx, "vhp_sweep_maps_batch", map_idx, s0, n); r != VHP_OK) return r;
    return sweep_maps_batch_device(ctx, ctx->d_src.get(), ctx->d_map_idx.get(), n, dtype, ctx->d_out.get(), {0, ctx->timing});
  });
  if (rc != VHP_OK || n_src == 0) return rc;
  rc = vhp_sync(ctx);
  zero_rejected_fields(ctx->maps, src_xy, map_idx, n_src, out_host, field);
  return rc;
}

int vhp_raycast_all(vhp_ctx* ctx, int src_x, int src_y, double* out_host) {
  if (!ctx || !out_host) return fail(ctx, VHP_ERR_ARG, "vhp_raycast_all: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_raycast_all: no map set");
  if (src_x < 0 || src_y < 0 || src_x >= ctx->map.nx || src_y >= ctx->map.ny) return fail(ctx, VHP_ERR_SOURCE_OOB, "source outside the grid");
  VHP_ON_DEVICE(ctx);
  const size_t cells = (size_t)ctx->map.nx * ctx->map.ny;
  VHP_HIP(ctx->d_out.grow(cells * 8));
  double* d = static_cast<double*>(ctx->d_out.get());
  const unsigned blocks = (unsigned)((cells + 255) / 256);
  VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(vhp::vhp_fill_f64, dim3(blocks), dim3(256), 0, ctx->stream, d, 1.0, cells);
  hipLaunchKernelGGL(vhp::vhp_raycast, dim3(blocks), dim3(256), 0, ctx->stream, ctx->map.nx, ctx->map.ny, ctx->d_occ.get(), src_x, src_y, d);
  VHP_HIP(hipGetLastError());
  VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed.events();
  VHP_HIP(hipMemcpyAsync(out_host, d, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  return VHP_OK;
}

// ---- ray casting for batches of sources, and line of sight (vhp_raycast.hip) ------------------------------------------------------
int vhp_raycast_batch(vhp_ctx* ctx, const int32_t* src_xy, int n_src, int dtype, void* out_host) {
  return raycast_host(ctx, "vhp_raycast_batch", false, src_xy, nullptr, n_src, dtype, out_host);
}
int vhp_raycast_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, int n_src, int dtype, void* d_out) {
  return raycast_device(ctx, "vhp_raycast_batch_device", false, d_src_xy, nullptr, n_src, dtype, d_out);
}
int vhp_raycast_maps_batch(vhp_ctx* ctx, const int32_t* src_xy, const int32_t* map_idx, int n_src, int dtype, void* out_host) {
  return raycast_host(ctx, "vhp_raycast_maps_batch", true, src_xy, map_idx, n_src, dtype, out_host);
}
int vhp_raycast_maps_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out) {
  return raycast_device(ctx, "vhp_raycast_maps_batch_device", true, d_src_xy, d_map_idx, n_src, dtype, d_out);
}

int vhp_line_of_sight_device(vhp_ctx* ctx, const int32_t* d_pairs_xyxy, int n_pairs, int32_t* d_hit_xy) {
  if (!ctx || !d_pairs_xyxy || !d_hit_xy || n_pairs < 0) return fail(ctx, VHP_ERR_ARG, "vhp_line_of_sight_device: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_line_of_sight_device: no map set");
  if ((reinterpret_cast<uintptr_t>(d_pairs_xyxy) | reinterpret_cast<uintptr_t>(d_hit_xy)) & 3)
    return fail(ctx, VHP_ERR_ARG, "vhp_line_of_sight_device: a buffer is not aligned to its element type");
  if (n_pairs == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  const hipError_t e = vhp::launch_line_of_sight(packed_occ(ctx->map), ctx->map.nx, ctx->map.ny, d_pairs_xyxy, n_pairs, d_hit_xy, ctx->d_err.get(), ctx->stream);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("vhp_line_of_sight_device: ") + hipGetErrorString(e));
  VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed.events();
  return VHP_OK;
}

int vhp_line_of_sight(vhp_ctx* ctx, const int32_t* pairs_xyxy, int n_pairs, int32_t* hit_xy) {
  if (!ctx || !pairs_xyxy || !hit_xy || n_pairs < 0) return fail(ctx, VHP_ERR_ARG, "vhp_line_of_sight: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_line_of_sight: no map set");
  if (n_pairs == 0) return VHP_OK;
  VHP_ON_DEVICE(ctx);
  // (pairs in the source scratch, hits in the output scratch: 16 and 8 bytes a pair, one copy each way)
  hipError_t e = ctx->d_src.grow((size_t)n_pairs * 4 * sizeof(int32_t));
  if (e == hipSuccess) e = ctx->d_out.grow((size_t)n_pairs * 2 * sizeof(int32_t));
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("vhp_line_of_sight: scratch: ") + hipGetErrorString(e));
  VHP_HIP(hipMemcpyAsync(ctx->d_src.get(), pairs_xyxy, (size_t)n_pairs * 4 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  const int rc = vhp_line_of_sight_device(ctx, ctx->d_src.get(), n_pairs, static_cast<int32_t*>(ctx->d_out.get()));
  if (rc != VHP_OK) return rc;
  VHP_HIP(hipMemcpyAsync(hit_xy, ctx->d_out.get(), (size_t)n_pairs * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  return vhp_sync(ctx);
}

// ---- max-union + arg-source of a batch of fields (vhp_union.hip.h) ---------------------------------------------------
static int union_common(vhp_ctx* ctx, const char* who, const void* d_fields, int n, int dtype, long long stride, const int32_t* d_labels, int first_index,
                        void* d_best, int32_t* d_arg) {
  if (!ctx || !d_best || !d_arg || n < 0 || (n > 0 && !d_fields)) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad argument");
  if (dtype != VHP_F64 && dtype != VHP_F32) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": bad dtype");
  if (ctx->map.nx <= 0) return fail(ctx, VHP_ERR_NO_MAP, std::string(who) + ": no map set (the grid's size is the map's)");
  const long long cells = (long long)ctx->map.nx * ctx->map.ny;
  if (stride == 0) stride = cells;
  if (stride < cells) return fail(ctx, VHP_ERR_ARG, std::string(who) + ": field_stride is smaller than a field");
  const size_t el = dtype == VHP_F64 ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d_fields) % el || reinterpret_cast<uintptr_t>(d_best) % el || reinterpret_cast<uintptr_t>(d_arg) % 4)
    return fail(ctx, VHP_ERR_ARG, std::string(who) + ": a pointer is not aligned to its element type");
  VHP_ON_DEVICE(ctx);
  // (not timed: ev0 / ev1 keep bracketing the most recent sweep or planner call, vhp_last_elapsed_ms)
  const hipError_t e = dtype == VHP_F64 ? vhp::launch_union<double>(d_fields, n, stride, d_labels, first_index, cells, d_best, d_arg, ctx->n_cus, ctx->stream)
                                        : vhp::launch_union<float>(d_fields, n, stride, d_labels, first_index, cells, d_best, d_arg, ctx->n_cus, ctx->stream);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return VHP_OK;
}

int vhp_union_fields_device(vhp_ctx* ctx, const void* d_fields, int n_fields, int dtype, int first_index, void* d_best, int32_t* d_arg) {
  return union_common(ctx, "vhp_union_fields_device", d_fields, n_fields, dtype, ctx ? ctx->opt_field_stride : 0, nullptr, first_index, d_best, d_arg);
}

int vhp_union_partials_device(vhp_ctx* ctx, const void* d_bests, const int32_t* d_args, int n_parts, int dtype, void* d_best, int32_t* d_arg) {
  if (n_parts > 0 && !d_args) return fail(ctx, VHP_ERR_ARG, "vhp_union_partials_device: bad argument");
  return union_common(ctx, "vhp_union_partials_device", d_bests, n_parts, dtype, 0, d_args, 0, d_best, d_arg);
}

// ---- MATLAB-flavoured variants (vhp_variant.hip.h) -------------------------------------------------------------------
static int variant_launch_sweep(vhp_ctx* ctx, const int32_t* d_src, int n_src, double alpha, double fac, double* d_out) {
  const size_t lds = (size_t)3 * (std::max(ctx->map.nx, ctx->map.ny) + 1) * sizeof(double);
  auto k = vhp::variant::vhp_variant_sweep;
  hipError_t e = raise_lds_limit(ctx, reinterpret_cast<const void*>(k), lds);
  if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("variant sweep: ") + hipGetErrorString(e));
  hipLaunchKernelGGL(k, dim3((unsigned)(4 * n_src)), dim3(1024), lds, ctx->stream, ctx->map.nx, ctx->map.ny, ctx->d_occ.get(), d_src, d_out,
                     (long long)ctx->map.nx * ctx->map.ny, alpha, fac, ctx->d_err.get());
  VHP_HIP(hipGetLastError());
  return VHP_OK;
}

int vhp_sweep_batch_variant(vhp_ctx* ctx, const int32_t* src_xy, int n_src, double alpha, double fac, double* out_host) {
  if (!ctx || !src_xy || !out_host || n_src < 0 || !(fac > 0)) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_variant: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_batch_variant: no map set");
  if (std::max(ctx->map.nx, ctx->map.ny) > 4096) return fail(ctx, VHP_ERR_TOO_LARGE, "variant sweeps: grid side above 4096");
  return stage_batch(ctx, "vhp_sweep_batch_variant", src_xy, n_src, 8, out_host,
                     [&](int n) { return variant_launch_sweep(ctx, ctx->d_src.get(), n, alpha, fac, static_cast<double*>(ctx->d_out.get())); });
}

int vhp_sweep_batch_offset(vhp_ctx* ctx, const int32_t* src_xy, int n_src, double offset, double* out_host) {
  if (!ctx || !src_xy || !out_host || n_src < 0 || !(offset >= 0)) return fail(ctx, VHP_ERR_ARG, "vhp_sweep_batch_offset: bad argument");
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_sweep_batch_offset: no map set");
  if (std::max(ctx->map.nx, ctx->map.ny) > 4096) return fail(ctx, VHP_ERR_TOO_LARGE, "offset sweeps: grid side above 4096");
  const size_t cells = (size_t)ctx->map.nx * ctx->map.ny;
  const size_t lds = (size_t)3 * (std::max(ctx->map.nx, ctx->map.ny) + 1) * sizeof(double);
  auto k = vhp::variant::vhp_offset_sweep;
  bool raised = false;
  return stage_batch(ctx, "vhp_sweep_batch_offset", src_xy, n_src, 8, out_host, [&](int n) -> int {
    if (!raised) {  // (once per call, on the context's device)
      hipError_t e = raise_lds_limit(ctx, reinterpret_cast<const void*>(k), lds);
      if (e != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("offset sweep: ") + hipGetErrorString(e));
      raised = true;
    }
    VHP_HIP(hipMemsetAsync(ctx->d_out.get(), 0, (size_t)n * cells * 8, ctx->stream));  // a freshly reset() solver
    hipLaunchKernelGGL(k, dim3((unsigned)(4 * n)), dim3(1024), lds, ctx->stream, ctx->map.nx, ctx->map.ny, ctx->d_occ.get(), ctx->d_src.get(),
                       static_cast<double*>(ctx->d_out.get()), (long long)cells, offset, ctx->d_err.get());
    VHP_HIP(hipGetLastError());
    return VHP_OK;
  });
}

int vhp_planner_solve_variant(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, double alpha,
                              uint64_t max_iter, uint64_t* label, double* map_builder, double* local, int32_t* waypoints_xy,
                              uint32_t* n_waypoints) {
  using namespace vhp::variant;
  if (!ctx) return VHP_ERR_ARG;
  if (!ctx->map.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, "vhp_planner_solve_variant: no map set");
  const int nx = ctx->map.nx, ny = ctx->map.ny;
  if (std::max(nx, ny) > 4096) return fail(ctx, VHP_ERR_TOO_LARGE, "variant planner: grid side above 4096");
  if ((unsigned)start_x >= (unsigned)nx || (unsigned)start_y >= (unsigned)ny) return fail(ctx, VHP_ERR_START_OOB, "Start point is out of bounds.");
  if ((unsigned)end_x >= (unsigned)nx || (unsigned)end_y >= (unsigned)ny) return fail(ctx, VHP_ERR_END_OOB, "End point is out of bounds.");
  if (max_iter > (1u << 20)) return fail(ctx, VHP_ERR_ARG, "max_iter too large");
  VHP_ON_DEVICE(ctx);
  const size_t cells = (size_t)nx * ny;
  // (the solve's own state, gone however the function is left)
  vhp::DevBuf<double> uni, loc;
  vhp::DevBuf<uint32_t> lab;
  vhp::DevBuf<unsigned long long> lab64;
  vhp::DevBuf<int32_t> way;
  vhp::DevBuf<PlannerCtl> ctl;
  VHP_HIP(uni.grow(cells * 8));
  VHP_HIP(loc.grow(cells * 8));
  VHP_HIP(lab.grow(cells * 4));
  VHP_HIP(lab64.grow(cells * 8));
  VHP_HIP(way.grow(2 * (size_t)(max_iter + 3) * sizeof(int32_t)));
  VHP_HIP(ctl.grow(sizeof(PlannerCtl)));
  double *const d_uni = uni.get(), *const d_loc = loc.get();
  uint32_t* const d_lab = lab.get();
  unsigned long long* const d_lab64 = lab64.get();
  int32_t* const d_way = way.get();
  PlannerCtl* const d_ctl = ctl.get();
  VHP_HIP(hipMemsetAsync(d_uni, 0, cells * 8, ctx->stream));
  VHP_HIP(hipMemsetAsync(d_lab, 0xff, cells * 4, ctx->stream));
  const int32_t w0[2] = {start_x, start_y};
  const PlannerCtl c0{1, 0, 0, 0};
  const uint32_t zero = 0;
  VHP_HIP(hipMemcpyAsync(d_way, w0, sizeof(w0), hipMemcpyHostToDevice, ctx->stream));
  VHP_HIP(hipMemcpyAsync(d_ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, ctx->stream));
  VHP_HIP(hipMemcpyAsync(d_lab + ((size_t)start_y * nx + start_x), &zero, 4, hipMemcpyHostToDevice, ctx->stream));  // lightSource_enum(start) = 1
  const unsigned eb = (unsigned)((cells + 255) / 256);
  PlannerCtl h{};
  for (;;) {
    // sweep from the current waypoint (d_way[2*iter]), union + labels, stop test
    int rc = variant_launch_sweep(ctx, d_way + 2 * h.iter, 1, alpha, 1.0, d_loc);
    if (rc != VHP_OK) return rc;
    hipLaunchKernelGGL(vhp_variant_update, dim3(eb), dim3(256), 0, ctx->stream, d_loc, d_uni, d_lab, cells, threshold, d_ctl);
    hipLaunchKernelGGL(vhp_variant_check, dim3(1), dim3(64), 0, ctx->stream, d_loc, nx, end_x, end_y, threshold, d_ctl);
    hipLaunchKernelGGL(vhp_variant_pick, dim3(1), dim3(1024), 0, ctx->stream, d_uni, nx, ny, end_x, end_y, threshold,
                       (unsigned long long)max_iter, d_way, d_ctl);
    VHP_HIP(hipGetLastError());
    VHP_HIP(hipMemcpyAsync(&h, d_ctl, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    VHP_HIP(hipStreamSynchronize(ctx->stream));
    if (h.done) break;
  }
  if (n_waypoints) *n_waypoints = (uint32_t)h.n_way;
  if (waypoints_xy) VHP_HIP(hipMemcpyAsync(waypoints_xy, d_way, 2 * (size_t)h.n_way * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (label) {
    hipLaunchKernelGGL(vhp_variant_labels_to_u64, dim3(eb), dim3(256), 0, ctx->stream, d_lab, d_lab64, cells, ~0ull);
    VHP_HIP(hipMemcpyAsync(label, d_lab64, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (map_builder) VHP_HIP(hipMemcpyAsync(map_builder, d_uni, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (local) VHP_HIP(hipMemcpyAsync(local, d_loc, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  if (h.status == VHP_ERR_MAX_ITER) ctx->err = "variant planner: max_iter reached";
  if (h.status == VHP_ERR_NOTHING_LIT) ctx->err = "variant planner: no candidate above the threshold";
  return h.status;
}

int vhp_timing(vhp_ctx* ctx, int enable) {
  if (!ctx) return VHP_ERR_ARG;
  ctx->timing = enable != 0;
  // The ring of stamp slots for `enable` timed launches between two vhp_timing_collect calls (64 where the caller names no number);
  // it only grows, and only while no timed launch is waiting to be collected.  Launches beyond it are timed by event pairs.
  if (const int want = enable > 1 ? enable : 64; enable && VHP_TIMING_STAMPS && ctx->clock_khz > 0 && ctx->ring.slots() < want && ctx->ring.live() == 0) {
    VHP_ON_DEVICE(ctx);
    read_last_stamps(ctx);  // (the array moves: a launch that vhp_last_elapsed_ms may still be asked about is read first)
    ctx->ring.resize(want, ctx->n_cus);
    if (const hipError_t es = allocate_stamps(ctx); es != hipSuccess) {
      ctx->ring.resize(0, ctx->n_cus);
      VHP_HIP(es);
    }
  }
  if (enable > 1) {  // pre-create `enable` event pairs so that no launch inside a timed loop has to
    VHP_ON_DEVICE(ctx);
    while ((int)ctx->event_pool.size() < enable) {
      hipEvent_t a = nullptr, b = nullptr;
      VHP_HIP(create_timing_event(&a));
      if (const hipError_t eb = create_timing_event(&b); eb != hipSuccess) {
        (void)hipEventDestroy(a);
        VHP_HIP(eb);
      }
      ctx->event_pool.push_back({a, b});
    }
  }
  return VHP_OK;
}

namespace {
// vhp_set_option's int keys: the values a key takes (min .. max, and `ok` where the domain is no interval), what a refusal says and
// where the value goes.  flag: any value, kept as 0 / 1.
struct OptionKey {
  const char* key;
  int min, max;
  const char* message;
  int& (*at)(vhp_ctx*);
  bool (*ok)(int) = nullptr;
  bool flag = false;
};
const OptionKey kOptionKeys[] = {
    {"rows_per_lane", 0, 4, "rows_per_lane: 0, 1, 2 or 4", [](vhp_ctx* c) -> int& { return c->opt_rows_per_lane; }, [](int v) { return v != 3; }},
    {"strips", 0, 8, "strips: 0..8", [](vhp_ctx* c) -> int& { return c->opt_strips; }},
    {"multi_round", INT_MIN, INT_MAX, "", [](vhp_ctx* c) -> int& { return c->opt_multi; }, nullptr, true},
    {"slide", -1, 1, "slide: -1, 0 or 1", [](vhp_ctx* c) -> int& { return c->opt_slide; }},
    {"pack", INT_MIN, INT_MAX, "", [](vhp_ctx* c) -> int& { return c->opt_pack; }, nullptr, true},
    {"lat_workgroups", 0, 8, "lat_workgroups: 0 (automatic), 1, 2, 4 or 8", [](vhp_ctx* c) -> int& { return c->opt_lat_workgroups; }, [](int v) { return v <= 2 || v == 4 || v == 8; }},
    {"kernel", 0, 4, "kernel: 0 auto, 1 fronts, 3 pool, 4 latency (2, the streaming sweep, was retired)", [](vhp_ctx* c) -> int& { return c->opt_kernel; }, [](int v) { return v != 2; }},
    {"pool_claim_ahead", -1, 64, "pool_claim_ahead: -1 (automatic) .. 64", [](vhp_ctx* c) -> int& { return c->opt_pool.claim_ahead; }},
    {"pool_heads", 0, 16, "pool_heads: 0 (automatic) .. 16", [](vhp_ctx* c) -> int& { return c->opt_pool.heads; }},
    {"pool_tail_pct", 0, 100, "pool_tail_pct: 0 (automatic) .. 100", [](vhp_ctx* c) -> int& { return c->opt_pool.tail_pct; }},
    {"pool_early_ctx", 0, 16, "pool_early_ctx: 0 (automatic) .. 16", [](vhp_ctx* c) -> int& { return c->opt_pool.early_ctx; }},
    {"pool_late_pct", 0, 100, "pool_late_pct: 0 (automatic) .. 100", [](vhp_ctx* c) -> int& { return c->opt_pool.late_pct; }},
    {"pool_busy_cap", 0, 16, "pool_busy_cap: 0 (automatic) .. 16", [](vhp_ctx* c) -> int& { return c->opt_pool.busy_cap; }},
    {"pool_contexts", 0, 16, "pool_contexts: 0 (automatic) .. 16", [](vhp_ctx* c) -> int& { return c->opt_pool.contexts; }},
    {"pool_static_round", 0, 2, "pool_static_round: 0, 1 or 2", [](vhp_ctx* c) -> int& { return c->opt_pool.static_round; }},
    {"planner_batch_group", 0, vhp::kBatchMaxGroup, "planner_batch_group: 0 (automatic) .. 32", [](vhp_ctx* c) -> int& { return c->opt_planner_batch_group; }},
    {"alloc_budget_pct", 1, 90, "alloc_budget_pct: 1 .. 90 (per cent of the free device memory)", [](vhp_ctx* c) -> int& { return c->opt_alloc_budget_pct; }},
};
}  // namespace

int vhp_set_option(vhp_ctx* ctx, const char* key, long long value) {
  if (!ctx || !key) return VHP_ERR_ARG;
  const std::string k(key);
  const int v = (int)value;
  // (the one key that takes all 64 bits of its value)
  if (k == "field_stride") { if (value < 0) return fail(ctx, VHP_ERR_ARG, "field_stride: 0 (packed) or elements per field"); ctx->opt_field_stride = value; return VHP_OK; }
  for (const OptionKey& o : kOptionKeys) {
    if (k != o.key) continue;
    if (v < o.min || v > o.max || (o.ok && !o.ok(v))) return fail(ctx, VHP_ERR_ARG, o.message);
    o.at(ctx) = o.flag ? v != 0 : v;
    return VHP_OK;
  }
  return fail(ctx, VHP_ERR_ARG, "vhp_set_option: unknown key '" + k + "'");
}

int vhp_last_sweep_kernel(const vhp_ctx* ctx) { return ctx ? ctx->last_kernel : 0; }

int vhp_timing_collect(vhp_ctx* ctx, float* ms_out, int cap, int* n) {
  if (!ctx || !n || cap < 0 || (cap > 0 && !ms_out)) return VHP_ERR_ARG;
  VHP_ON_DEVICE(ctx);
  int k = 0, bad = 0;
  // the stamped launches: the streams they went out on synchronised, then the ring's slots that are out in one copy (two where they
  // wrap); if that fails none of them can be read
  bool stamps_ok = true;
  int n_stamped = 0;
  {
    void* synced = nullptr;
    for (auto& t : ctx->timed_launches) {
      if (!t.st.stamped()) continue;
      if ((n_stamped++ == 0 || t.st.stream != synced) && hipStreamSynchronize(static_cast<hipStream_t>(t.st.stream)) != hipSuccess) stamps_ok = false;
      synced = t.st.stream;
    }
    int first[2], count[2];
    const int n_runs = n_stamped ? ctx->ring.runs(first, count) : 0;
    for (int r = 0; r < n_runs; ++r)
      if (copy_stamp_slots(ctx, first[r], count[r]) != hipSuccess) stamps_ok = false;
    if (!stamps_ok) (void)hipGetLastError();
  }
  for (auto& t : ctx->timed_launches) {
    float ms = 0.f;
    bool ok;
    if (t.st.stamped()) {
      vhp::stamps::Time tm;
      if (stamps_ok) tm = vhp::stamps::reduce(ctx->h_stamps.data() + ctx->ring.slot_offset(t.st.slot), t.st, ctx->clock_khz);
      ctx->timed.read(t.st.tag, tm);  // (vhp_last_elapsed_ms reports the same number once the slot has gone back)
      ok = tm.ok;
      ms = tm.ms;
    } else {
      // a pair that cannot be read (e.g. never recorded) is dropped, not left to fail every later call
      ok = hipEventSynchronize(t.ev.second) == hipSuccess && hipEventElapsedTime(&ms, t.ev.first, t.ev.second) == hipSuccess;
      if (!ok) (void)hipGetLastError();
      ctx->event_pool.push_back(t.ev);  // recycled by the next timed launches
    }
    if (ok) {
      if (k < cap) ms_out[k] = ms;
      ++k;
    } else {
      ++bad;
    }
  }
  ctx->ring.release(n_stamped);
  ctx->timed_launches.clear();
  *n = std::min(k, cap);
  if (bad) return fail(ctx, VHP_ERR_HIP, "vhp_timing_collect: " + std::to_string(bad) + " timed launch(es) could not be read");
  return VHP_OK;
}

// ---- vhp_probe_stores: what the memory behind a buffer does with whole and with split lines (a measurement aid) -----------
namespace {
// Persistent wavefronts pull tasks; a task = 1000 rows of 8000 B (the C3 field's pitch: every other row starts half a 128-byte
// line off the grid) x a band of 1 KB; a store instruction = one row of the band, plain stores.  split = 0: every piece moved
// onto the line grid (whole lines only); split = 1: the pieces where they fall (two half lines per odd row).
__global__ void __launch_bounds__(256) vhp_store_probe_kernel(char* out, int n_tasks, int split, unsigned* counter) {
  extern __shared__ double probe_lds[];
  const int lane = threadIdx.x & 63;
  const double2 val = make_double2(0.0, 0.0);
  for (;;) {
    unsigned t = 0;
    if (lane == 0) t = atomicAdd(counter, 1u);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= (unsigned)n_tasks) break;
    const unsigned blk = t / 7u, band = t - blk * 7u;
    char* base = out + (size_t)blk * 8000000u + (size_t)band * 1024u + (size_t)lane * 16u;
    for (int row = 0; row < 1000; ++row) *reinterpret_cast<double2*>(base + (size_t)row * 8000u + ((!split && (row & 1)) ? 64 : 0)) = val;
  }
}
}  // namespace

int vhp_probe_stores(vhp_ctx* ctx, void* d_buf, unsigned long long bytes, float* whole_lines_TBps, float* split_lines_TBps) {
  if (!ctx || !d_buf || !whole_lines_TBps || !split_lines_TBps) return VHP_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(d_buf) & 127u) != 0) return fail(ctx, VHP_ERR_ARG, "vhp_probe_stores: the buffer must start on a 128-byte line");
  const unsigned long long blocks = bytes / 8000000ull;
  if (blocks < 16) return fail(ctx, VHP_ERR_ARG, "vhp_probe_stores: needs at least 128 MB to say anything about the memory");
  VHP_ON_DEVICE(ctx);
  const int n_tasks = (int)std::min<unsigned long long>(blocks, 2048) * 7;
  // (the task counter lives with the context: vhp_alloc_output probes up to 64 buffers, and a hipFree per probe synchronises the device;
  // the timing pair is the context's own ev0 / ev1 -- nothing here can leak on an early return)
  VHP_HIP(ctx->d_probe_counter.grow(8));
  float res[2] = {0.f, 0.f};
  for (int split = 0; split < 2; ++split) {
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
      VHP_HIP(hipMemsetAsync(ctx->d_probe_counter.get(), 0, 4, ctx->stream));
      VHP_HIP(hipEventRecord(ctx->ev0, ctx->stream));
      // three workgroups of four wavefronts per CU (52 KB of LDS each keeps a fourth out): what a launch of the pool sweep holds
      hipLaunchKernelGGL(vhp_store_probe_kernel, dim3((unsigned)ctx->n_cus * 3), dim3(256), 52 * 1024, ctx->stream, static_cast<char*>(d_buf), n_tasks, split, ctx->d_probe_counter.get());
      VHP_HIP(hipGetLastError());
      VHP_HIP(hipEventRecord(ctx->ev1, ctx->stream));
      VHP_HIP(hipEventSynchronize(ctx->ev1));
      float ms = 0.f;
      VHP_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      if (rep > 0 && ms < best) best = ms;
    }
    res[split] = (float)((double)n_tasks * 1000.0 * 1024.0 / ((double)best * 1e-3) / 1e12);
  }
  ctx->timed.nothing();  // (ev0 / ev1 no longer bracket a sweep)
  *whole_lines_TBps = res[0];
  *split_lines_TBps = res[1];
  return VHP_OK;
}

int vhp_alloc_output(vhp_ctx* ctx, unsigned long long bytes, int max_candidates, void** d_buf, float* whole_lines_TBps, float* split_lines_TBps,
                     int* n_tried) {
  if (!ctx || !d_buf || bytes == 0 || max_candidates < 1) return fail(ctx, VHP_ERR_ARG, "vhp_alloc_output: bad argument");
  VHP_ON_DEVICE(ctx);
  *d_buf = nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  size_t free_b = 0, total_b = 0;
  VHP_HIP(hipMemGetInfo(&free_b, &total_b));
  // Every candidate stays allocated until the choice is made -- a freed one would be handed out again.  The search is a guest on
  // the device: what it holds at once stays within "alloc_budget_pct" (default 25) per cent of the memory that is free when it
  // starts, it ends on the first buffer of the fast kind, and it gives up after 8 candidates in a row that are no better than the
  // best so far (where the fast kind is rare a longer search mostly finds more of the same).
  const unsigned long long budget = (unsigned long long)free_b / 100ull * (unsigned long long)ctx->opt_alloc_budget_pct;
  const int cap = (int)std::min<unsigned long long>((unsigned long long)std::min(max_candidates, 64), std::max<unsigned long long>(1, budget / bytes));
  const bool probed = bytes >= 16ull * 8000000ull;   // (vhp_probe_stores says nothing about less than 128 MB)
  struct Held {  // (whatever way this function is left, only the keeper survives)
    std::vector<void*> v;
    void* keep = nullptr;
    ~Held() { for (void* q : v) if (q != keep) (void)hipFree(q); }
  } cand;
  int best = -1, tried = 0, since_best = 0;
  float best_w = 0.f, best_s = 0.f;
  for (int k = 0; k < cap; ++k) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
    cand.v.push_back(p);
    ++tried;
    float w = 0.f, sp = 0.f;
    if (probed) {
      const int rc = vhp_probe_stores(ctx, p, bytes, &w, &sp);
      if (rc != VHP_OK) return rc;
    }
    // (the two rates move together -- 4.9 / 3.6 on the slow kind, 6.0 / 5.3 on the fast, anything between on a buffer that straddles
    // both --: their sum ranks the candidates; an improvement is more than the probe's own scatter of ~0.05 TB/s)
    if (best < 0 || w + sp > best_w + best_s + 0.05f) { best = k; best_w = w; best_s = sp; since_best = 0; } else ++since_best;
    if (!probed || (w >= 5.5f && sp >= 4.6f)) break;   // the fast kind (5.6-6.1 / 4.6-5.4 by box): nothing better to find
    if (since_best >= 8) break;
  }
  ctx->last_alloc_peak_bytes = (unsigned long long)tried * bytes;
  ctx->last_alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if (best < 0) return fail(ctx, VHP_ERR_HIP, "vhp_alloc_output: out of device memory");
  cand.keep = cand.v[best];
  ctx->placed.push_back(cand.keep);
  *d_buf = cand.keep;
  if (whole_lines_TBps) *whole_lines_TBps = best_w;
  if (split_lines_TBps) *split_lines_TBps = best_s;
  if (n_tried) *n_tried = tried;
  return VHP_OK;
}

int vhp_alloc_output_cost(const vhp_ctx* ctx, double* search_ms, unsigned long long* peak_bytes) {
  if (!ctx) return VHP_ERR_ARG;
  if (search_ms) *search_ms = ctx->last_alloc_ms;
  if (peak_bytes) *peak_bytes = ctx->last_alloc_peak_bytes;
  return VHP_OK;
}

int vhp_free_output(vhp_ctx* ctx, void* d_buf) {
  if (!ctx || !d_buf) return VHP_ERR_ARG;
  auto it = std::find(ctx->placed.begin(), ctx->placed.end(), d_buf);
  if (it == ctx->placed.end()) return fail(ctx, VHP_ERR_ARG, "vhp_free_output: not a buffer of vhp_alloc_output of this context");
  VHP_ON_DEVICE(ctx);
  VHP_HIP(hipStreamSynchronize(ctx->stream));
  ctx->placed.erase(it);
  VHP_HIP(hipFree(d_buf));
  return VHP_OK;
}

int vhp_last_elapsed_ms(vhp_ctx* ctx, float* ms) {
  if (!ctx || !ms) return VHP_ERR_ARG;
  if (ctx->timed.state == vhp::stamps::Last::kNothing) return fail(ctx, VHP_ERR_ARG, "nothing timed yet");
  VHP_ON_DEVICE(ctx);
  if (ctx->timed.state == vhp::stamps::Last::kEvents) {
    VHP_HIP(hipEventSynchronize(ctx->ev1));
    VHP_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return VHP_OK;
  }
  read_last_stamps(ctx);  // (a launch that has been read -- here before, or by vhp_timing_collect -- keeps its number)
  if (!ctx->timed.time.ok) return fail(ctx, VHP_ERR_HIP, "vhp_last_elapsed_ms: the launch's timestamps could not be read");
  *ms = ctx->timed.time.ms;
  return VHP_OK;
}

int vhp_planner_solve(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold,
                      uint64_t max_iter, uint64_t* came_from, double* vis_global, double* vis_local,
                      int32_t* pivots_xy, uint32_t* n_pivots) {
  // one source per sweep: the latency sweep wherever a batch of one would take it (94 against 67 us per sweep at 690^2)
  return planner_call(ctx, "vhp_planner_solve", 1, 4, [&](const vhp::DevMap& pm, const vhp::SweepPlan& plan, std::string* msg) {
    ctx->pl.lat_sweep = nullptr;
    if (plan.kernel == 4)
      ctx->pl.lat_sweep = [ctx](const int32_t* pivots, const int* nb, const int* done, const int* rec, double* out, bool dark_unwritten) {
        vhp::LatLaunch l;
        l.src_index = nb;
        l.skip = done;
        l.pivot_rec = rec;
        l.dark_unwritten = dark_unwritten;
        // (the option's stride, not "packed": one field is written at d_out whatever the stride, but an odd stride takes the sweep's
        // build for odd pitches -- vhp_lat.hip lat_needs_odd)
        return launch_batch_sweep<double>(ctx, ctx->map, pivots, 1, out, true, {ctx->opt_field_stride, false}, l);
      };
    // ... or the iteration as ONE launch (vhp_lat.hip vhp_planner_iteration) -- built in round 6, bit-exact, and SLOWER on this part: the
    // epilogue's workgroups sit behind other L2s than the sweep's, so the hand-off inside a launch costs an L2 write-back and an
    // invalidate (39.6 us per pivot on maze_6 against 22.8 with two launches; 32.6 with the local fields in uncached memory and no
    // fences, VHP_PLANNER_UNCACHED: profiles/r06_planner_one_kernel_ab.txt).  Only with VHP_PLANNER_ONE_KERNEL set in the environment.
    ctx->pl.lat_iteration = nullptr;
    static const bool one_kernel = std::getenv("VHP_PLANNER_ONE_KERNEL") != nullptr;
    if (ctx->pl.lat_sweep && one_kernel)
      ctx->pl.lat_iteration = [ctx](const vhp::PlannerDev& d) {
        vhp::LatLaunch l;
        l.pivot_rec = d.rec;
        l.dark_unwritten = true;
        l.planner_dev = &d;
        return launch_batch_sweep<double>(ctx, ctx->map, d.pivots, 1, d.vis_local, true, {ctx->opt_field_stride, false}, l);
      };
    return vhp::planner_solve(ctx->pl, pm, ctx->d_occ.get(), ctx->stream, ctx->ev0, ctx->ev1, start_x, start_y, end_x, end_y, threshold, max_iter,
                              came_from, vis_global, vis_local, pivots_xy, n_pivots, msg);
  });
}

int vhp_planner_solve_speculative(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, uint64_t max_iter, int k,
                                  int mode, uint64_t* came_from, double* vis_global, double* vis_local, int32_t* pivots_xy,
                                  uint32_t* n_pivots, int32_t* stats) {
  // k sources per launch: the latency sweep (8 k workgroups) wherever a batch of k would take it
  return planner_call(ctx, "vhp_planner_solve_speculative", k, (size_t)4 * vhp::kSpecMaxK,
                      [&](const vhp::DevMap& pm, const vhp::SweepPlan& plan, std::string* msg) {
    ctx->pl.lat_sweep_k = nullptr;
    if (plan.kernel == 4)
      ctx->pl.lat_sweep_k = [ctx](const int32_t* cand, int n, const int* slot_base, const int* run_if, const int* done, double* cache, bool dark_unwritten) {
        vhp::LatLaunch l;
        l.skip = done;
        l.slot_base = slot_base;
        l.run_if = run_if;
        l.dark_unwritten = dark_unwritten;
        return launch_batch_sweep<double>(ctx, ctx->map, cand, n, cache, true, {}, l);  // (the cache holds packed fields)
      };
    int st[3] = {0, 0, 0};
    const int rc = vhp::planner_solve_speculative(ctx->pl, ctx->spec, pm, ctx->d_occ.get(), ctx->stream, ctx->ev0, ctx->ev1, start_x, start_y, end_x, end_y,
                                                  threshold, max_iter, k, mode, came_from, vis_global, vis_local, pivots_xy, n_pivots, st, msg);
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2]; }
    return rc;
  });
}

int vhp_planner_solve_device(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, uint64_t max_iter,
                             uint32_t* n_pivots) {
  return vhp_planner_solve(ctx, start_x, start_y, end_x, end_y, threshold, max_iter, nullptr, nullptr, nullptr, nullptr, n_pivots);
}

int vhp_planner_results_device(vhp_ctx* ctx, const uint32_t** labels, const double** vis_global, const double** vis_local,
                               const int32_t** pivots_xy) {
  if (!ctx) return VHP_ERR_ARG;
  if (!ctx->pl.vis_global.get()) return fail(ctx, VHP_ERR_ARG, "vhp_planner_results_device: no planner solve has run on this map");
  if (labels) *labels = ctx->pl.label.get();
  if (vis_global) *vis_global = ctx->pl.vis_global.get();
  if (vis_local) *vis_local = ctx->pl.vis_local_out ? ctx->pl.vis_local_out : ctx->pl.vis_local.get();
  if (pivots_xy) *pivots_xy = ctx->pl.pivots.get();
  return VHP_OK;
}

// vhp_planner_solve_batch on the single map and, with `maps`, vhp_planner_solve_maps_batch on the stack (query q on map map_idx[q]).
static int solve_batch(vhp_ctx* ctx, bool maps, const int32_t* queries, const int32_t* map_idx, const double* thresholds, int n_queries,
                       uint64_t max_iter, int32_t* status, uint32_t* n_pivots) {
  if (!ctx) return VHP_ERR_ARG;
  const std::string who = maps ? "vhp_planner_solve_maps_batch" : "vhp_planner_solve_batch";
  if (n_queries < 1 || n_queries > vhp::kBatchMaxQueries) return fail(ctx, VHP_ERR_ARG, who + ": n_queries outside 1..64");
  if (!queries || (maps && !map_idx) || !thresholds || !status || !n_pivots) return fail(ctx, VHP_ERR_ARG, who + ": null array");
  if (max_iter > (1u << 24)) return fail(ctx, VHP_ERR_ARG, "max_iter too large");
  const auto [b, m, none_solved] = batch_on(ctx, maps);
  if (!m.rows.get()) return fail(ctx, VHP_ERR_NO_MAP, who + (maps ? ": no maps set" : ": no map set"));
  for (int q = 0; maps && q < n_queries; ++q)
    if (map_idx[q] < 0 || map_idx[q] >= m.n) return fail(ctx, VHP_ERR_ARG, who + ": query " + std::to_string(q) + ": map index outside the stack");
  VHP_ON_DEVICE(ctx);
  vhp::DevMap pm = dev_map(m);
  const int G = planner_batch_group_size(ctx, m, max_iter);
  b.lat_sweep = nullptr;
  b.front_sweep = nullptr;
  if (G > 0) {
    if (maps && !m.dmap.get()) {  // (the stack's diagonal maps: built once, by the first batch that sweeps them)
      VHP_HIP(m.dmap.grow(vhp::lat_diag_map_bytes(m.nx, m.ny) * m.n));
      const hipError_t e = vhp::lat_pack_diag_stack(m.rows.get(), m.n, m.nx, m.ny, m.wpr, m.dmap.get(), ctx->stream);
      if (e != hipSuccess) {
        m.dmap.reset();
        return fail(ctx, VHP_ERR_HIP, who + ": diagonal maps: " + hipGetErrorString(e));
      }
    }
    vhp::BatchState* bs = &b;
    vhp::PackedMaps* pk = &m;
    b.lat_sweep = [ctx, bs, pk](const int32_t* cand, const int32_t* d_map_idx, int n, double* out) {
      vhp::LatLaunch l;
      l.slot_base = reinterpret_cast<const int*>(bs->n_done.get() + 1);  // (a zero: field g of the launch is query g's)
      l.dark_unwritten = true;
      l.map_idx = d_map_idx;  // (null on the single map)
      return launch_batch_sweep<double>(ctx, *pk, cand, n, out, true, {}, l);  // (the queries' local fields are packed)
    };
    ctx->last_kernel = 4;
  } else {
    const vhp::SweepPlan plan = plan_for_grid(ctx, m, 1, true);
    hipError_t eb = vhp::attach_round_scratch(pm, plan.W * 64 * plan.R, 4, ctx->d_bnd);
    if (eb != hipSuccess) return fail(ctx, VHP_ERR_HIP, std::string("scratch: ") + hipGetErrorString(eb));
    // (where the latency sweep does not take a single source: vhp_planner_sweep, as planner_solve launches it)
    b.front_sweep = [ctx, pm, plan, pk = &m](const vhp::PlannerDev& d, int k) {
      vhp::DevMap mk = pm;  // (map k of the stack; k is 0 on the single map)
      mk.rows = vhp::map_rows(*pk, k);
      mk.cols = vhp::map_cols(*pk, k);
      auto raise_lds = [ctx](const void* fn, size_t bytes) { return raise_lds_limit(ctx, fn, bytes); };
      return vhp::with_sweep_shape(plan.R, plan.multi, [&](auto r, auto mr) {
        return vhp::launch_planner_kernel<r(), mr()>(vhp::vhp_planner_sweep<r(), mr()>, 4, plan.W, raise_lds, ctx->stream, mk, d);
      });
    };
    ctx->last_kernel = 1;
  }
  const vhp::BatchStack st{map_idx, m.rows.get(), vhp::map_rows(m, 1) - vhp::map_rows(m, 0), m.wpr};
  std::string msg;
  const int rc = vhp::planner_solve_batch(b, pm, maps ? nullptr : ctx->d_occ.get(), maps || ctx->h_occ.empty() ? nullptr : ctx->h_occ.data(), ctx->stream,
                                          ctx->ev0, ctx->ev1, queries, thresholds, n_queries, max_iter, G > 0 ? G : 1, status, n_pivots, &msg,
                                          maps ? &st : nullptr);
  ctx->timed.events();
  if (!msg.empty()) ctx->err = msg;
  return rc;
}

static int batch_results_device(vhp_ctx* ctx, const char* who, bool maps, int q, const uint32_t** labels, const double** vis_global,
                                const double** vis_local, const int32_t** pivots_xy) {
  if (!ctx) return VHP_ERR_ARG;
  int k = 0;
  if (int rc = batch_slot(ctx, who, maps, q, &k); rc != VHP_OK) return rc;
  vhp::batch_results_device(batch_on(ctx, maps).b, k, labels, vis_global, vis_local, pivots_xy);
  return VHP_OK;
}

static int batch_results(vhp_ctx* ctx, const char* who, bool maps, int q, uint64_t* came_from, double* vis_global, double* vis_local,
                         int32_t* pivots_xy) {
  if (!ctx) return VHP_ERR_ARG;
  int k = 0;
  if (int rc = batch_slot(ctx, who, maps, q, &k); rc != VHP_OK) return rc;
  VHP_ON_DEVICE(ctx);
  std::string msg;
  const int rc = vhp::batch_results_host(batch_on(ctx, maps).b, k, ctx->stream, came_from, vis_global, vis_local, pivots_xy, &msg);
  if (rc != VHP_OK) ctx->err = msg;
  return rc;
}

static int batch_group(const vhp::BatchState& b) { return b.solved ? b.group : 0; }

int vhp_planner_solve_batch(vhp_ctx* ctx, const int32_t* queries, const double* thresholds, int n_queries, uint64_t max_iter,
                            int32_t* status, uint32_t* n_pivots) {
  return solve_batch(ctx, false, queries, nullptr, thresholds, n_queries, max_iter, status, n_pivots);
}
int vhp_planner_solve_maps_batch(vhp_ctx* ctx, const int32_t* queries, const int32_t* map_idx, const double* thresholds, int n_queries,
                                 uint64_t max_iter, int32_t* status, uint32_t* n_pivots) {
  return solve_batch(ctx, true, queries, map_idx, thresholds, n_queries, max_iter, status, n_pivots);
}
int vhp_planner_batch_group(const vhp_ctx* ctx) { return ctx ? batch_group(ctx->batch) : 0; }
int vhp_planner_maps_batch_group(const vhp_ctx* ctx) { return ctx ? batch_group(ctx->maps_batch) : 0; }
int vhp_planner_batch_results_device(vhp_ctx* ctx, int q, const uint32_t** labels, const double** vis_global, const double** vis_local,
                                     const int32_t** pivots_xy) {
  return batch_results_device(ctx, "vhp_planner_batch_results_device", false, q, labels, vis_global, vis_local, pivots_xy);
}
int vhp_planner_maps_batch_results_device(vhp_ctx* ctx, int q, const uint32_t** labels, const double** vis_global, const double** vis_local,
                                          const int32_t** pivots_xy) {
  return batch_results_device(ctx, "vhp_planner_maps_batch_results_device", true, q, labels, vis_global, vis_local, pivots_xy);
}
int vhp_planner_batch_results(vhp_ctx* ctx, int q, uint64_t* came_from, double* vis_global, double* vis_local, int32_t* pivots_xy) {
  return batch_results(ctx, "vhp_planner_batch_results", false, q, came_from, vis_global, vis_local, pivots_xy);
}
int vhp_planner_maps_batch_results(vhp_ctx* ctx, int q, uint64_t* came_from, double* vis_global, double* vis_local, int32_t* pivots_xy) {
  return batch_results(ctx, "vhp_planner_maps_batch_results", true, q, came_from, vis_global, vis_local, pivots_xy);
}

int vhp_planner_batch_paths(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status) {
  return batch_paths(ctx, "vhp_planner_batch_paths", false, false, path_xy, cap, n_path, length, path_status);
}
int vhp_planner_batch_paths_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length, int32_t* d_path_status) {
  return batch_paths(ctx, "vhp_planner_batch_paths_device", false, true, d_path_xy, cap, d_n_path, d_length, d_path_status);
}
int vhp_planner_maps_batch_paths(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status) {
  return batch_paths(ctx, "vhp_planner_maps_batch_paths", true, false, path_xy, cap, n_path, length, path_status);
}
int vhp_planner_maps_batch_paths_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length,
                                        int32_t* d_path_status) {
  return batch_paths(ctx, "vhp_planner_maps_batch_paths_device", true, true, d_path_xy, cap, d_n_path, d_length, d_path_status);
}
int vhp_planner_path(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status) {
  return plain_path(ctx, "vhp_planner_path", false, path_xy, cap, n_path, length, path_status);
}
int vhp_planner_path_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length, int32_t* d_path_status) {
  return plain_path(ctx, "vhp_planner_path_device", true, d_path_xy, cap, d_n_path, d_length, d_path_status);
}

int vhp_planner_length_fields(vhp_ctx* ctx, int solve, int q_first, int n_q, double* length, uint32_t* n_path) {
  return length_fields(ctx, "vhp_planner_length_fields", false, solve, q_first, n_q, length, n_path);
}
int vhp_planner_length_fields_device(vhp_ctx* ctx, int solve, int q_first, int n_q, double* d_length, uint32_t* d_n_path) {
  return length_fields(ctx, "vhp_planner_length_fields_device", true, solve, q_first, n_q, d_length, d_n_path);
}
int vhp_planner_goal_paths(vhp_ctx* ctx, int solve, const int32_t* goals_qxy, int n_goals, int32_t* path_xy, uint32_t cap, uint32_t* n_path,
                           double* length, int32_t* path_status) {
  return goal_paths(ctx, "vhp_planner_goal_paths", false, solve, goals_qxy, n_goals, path_xy, cap, n_path, length, path_status);
}
int vhp_planner_goal_paths_device(vhp_ctx* ctx, int solve, const int32_t* d_goals_qxy, int n_goals, int32_t* d_path_xy, uint32_t cap,
                                  uint32_t* d_n_path, double* d_length, int32_t* d_path_status) {
  return goal_paths(ctx, "vhp_planner_goal_paths_device", true, solve, d_goals_qxy, n_goals, d_path_xy, cap, d_n_path, d_length, d_path_status);
}

// eval_d of visibilityBasedSolver.h:112-115 (host side, used only for the path length)
static inline double eval_d_host(int ax, int ay, int bx, int by) {
  return std::sqrt((double)(ax - bx) * (ax - bx) + (ay - by) * (ay - by));
}

int vhp_reconstruct_path(const uint64_t* came_from, const int32_t* pivots_xy, uint32_t n_pivots, int nx, int ny, int end_x,
                         int end_y, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length) {
  if (!came_from || !pivots_xy || nx <= 0 || ny <= 0) return VHP_ERR_ARG;
  if (end_x < 0 || end_y < 0 || end_x >= nx || end_y >= ny) return VHP_ERR_END_OOB;
  // walk labels back to the start: the label of a pivot's own cell is the pivot that
  // lit it, the start labels itself, so the walk stops when the label repeats.  Labels index
  // pivots_xy[0 .. n_pivots]; a consistent table needs at most n_pivots + 1 hops.
  std::vector<std::pair<int, int>> rev;
  int x = end_x, y = end_y;
  uint64_t t = came_from[(size_t)x + (size_t)y * nx];
  uint64_t t_old = std::numeric_limits<uint64_t>::max();
  while (t != t_old) {
    rev.push_back({x, y});
    t_old = t;
    if (t > n_pivots) return VHP_ERR_ARG;  // unlabelled cell (VHP_UNLABELLED) or a label outside the pivot list
    if (rev.size() > (size_t)n_pivots + 2) return VHP_ERR_ARG;  // the labels form a cycle: not a planner result
    x = pivots_xy[2 * t];
    y = pivots_xy[2 * t + 1];
    if (x < 0 || y < 0 || x >= nx || y >= ny) return VHP_ERR_ARG;
    t = came_from[(size_t)x + (size_t)y * nx];
  }
  rev.push_back({x, y});
  std::reverse(rev.begin(), rev.end());
  double total = 0.0;
  for (size_t k = 0; k + 1 < rev.size(); ++k)
    total += eval_d_host(rev[k].first, rev[k].second, rev[k + 1].first, rev[k + 1].second);
  if (n_path) *n_path = (uint32_t)rev.size();  // the size needed, also when it exceeds cap
  if (length) *length = total;
  if (path_xy) {
    if (rev.size() > cap) return VHP_ERR_TOO_LARGE;  // nothing written; *n_path says how many points there are
    for (size_t k = 0; k < rev.size(); ++k) {
      path_xy[2 * k] = rev[k].first;
      path_xy[2 * k + 1] = rev[k].second;
    }
  }
  return VHP_OK;
}

}  // extern "C"
