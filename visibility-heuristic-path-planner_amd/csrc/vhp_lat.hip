// vhp_lat.hip -- gfx950 build of the latency sweep (vhp_lat.hpp) and its launcher.
// Plain field stores here (not the batch kernels' non-temporal ones, vhp_lanes.hpp): a launch of this kernel writes a few fields
// that its caller reads right away -- the planner's epilogue, the host copy of a small batch -- out of the caches.
#define VHP_FIELD_STORE_PLAIN 1
#include "vhp_batch_launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "vhp.h"
#include "vhp_band.hpp"
#include "vhp_planner_dev.hip.h"

namespace vhp {
namespace pool {

// One workgroup per unit (octant of a quadrant of a source) of kLatWaves strip wavefronts (vhp_launch_plan.hpp, with LatWorkerT).

#ifdef VHP_DIAG_POOLPROF  // diagnostic builds only (tools/lat_timeline.py)
__device__ unsigned long long g_latprof[256 * 16 * 20];
__device__ unsigned long long g_lat_strip_times[64 * 48 * 4];
#endif

// wavefronts of a workgroup: kLatWaves sweepers and, in the band sweep, a storer beside each (16: four per SIMD, 128 vector registers)
constexpr int kLatThreads = 64 * kLatWaves * LatWorkerT<double, false>::kRoles;

// A launch's timestamp (vhp_stamps.hpp): the device's constant-rate clock and the launch's tag, one 16-byte store by the calling lane.
__device__ __forceinline__ void write_stamp(stamps::Entry* p, unsigned long long tag) {
  *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2((unsigned long long)wall_clock64(), tag);
}

// MULTI: the build for launches with more than one workgroup per unit (vhp_launch_plan.hpp lat_halves): its bands can read across workgroups
// stamp_begin: where workgroup g leaves the launch's begin stamp [g] as its first act (null: the launch's pre-kernel has left it, or the
// launch is not stamped); stamp_end: its end stamp [g], once all its wavefronts are done (null: not stamped)
template <typename OutT, bool ODD, bool MULTI>
__global__ void __launch_bounds__(kLatThreads, 1) vhp_lat_sweep(LatArgs<OutT> a, stamps::Entry* __restrict__ stamp_begin,
                                                                stamps::Entry* __restrict__ stamp_end) {
  if (stamp_begin && threadIdx.x == 0) write_stamp(stamp_begin + blockIdx.x, a.epoch);
  extern __shared__ double lds[];
  const Layout L = make_layout(kLatWaves, 1, a.m.nx, a.m.ny, kLatTilePitch);
#ifdef VHP_DIAG_POOLPROF
  const unsigned long long t_begin = wall_clock64();
#endif
  using WorkerT = LatWorkerT<OutT, ODD, MULTI>;
  WorkerT::clear(lds, L, (int)threadIdx.x, kLatThreads);
  __syncthreads();
  WorkerT wk;
  wk.init(a, lds, L, uniform((int)(threadIdx.x >> 6)));
  wk.run((int)blockIdx.x);
  if (stamp_end) {  // every wavefront waits for its own stores, the barrier, then one lane reads the clock
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) write_stamp(stamp_end + blockIdx.x, a.epoch);
  }
#ifdef VHP_DIAG_POOLPROF
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && threadIdx.x < 64 * 16) {
    unsigned long long* o = g_latprof + ((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 20;
    for (int k = 0; k < 16; ++k) o[k] = wk.prof[k];
    o[16] = t_begin;
    o[17] = wall_clock64();
  }
#endif
}

// The latency sweep on a stack of maps (fp64, the planner's fields): vhp_lat_sweep's band build with the STACK flag -- every unit reads
// its source's map index once, before its sweep, and moves its maps there (vhp_band.hpp BandWorker::run).  The stack is an argument of
// its own: LatArgs, and with it the eight instantiations above, stay as they are.
template <bool ODD, bool MULTI>
__global__ void __launch_bounds__(kLatThreads, 1) vhp_lat_maps_sweep(LatArgs<double> a, LatMapStack st) {
  extern __shared__ double lds[];
  const Layout L = make_layout(kLatWaves, 1, a.m.nx, a.m.ny, kLatTilePitch);
  using WorkerT = BandWorker<double, ODD, MULTI, true>;
  WorkerT::clear(lds, L, (int)threadIdx.x, kLatThreads);
  __syncthreads();
  WorkerT wk;
  wk.init(a, lds, L, uniform((int)(threadIdx.x >> 6)));
  wk.stk = st;
  wk.run((int)blockIdx.x);
}

// A whole planner iteration as ONE launch (the reference's loop body, src/visibilityBasedSolver.cpp:127-141 with updateVisibility()
// :379-565: sweep, union, labels, heuristic, next pivot): the first eight workgroups are the eight octants of the pivot's sweep, the
// others run the epilogue (vhp_planner_dev.hip.h) behind them -- the loads that do not depend on the sweep on their way while it runs,
// the local field read once the eight have counted themselves in.  (Until round 6: two launches per iteration, 1.7 us between them.)
constexpr int kPlanEpiBlocks = kEpilogueBlocks;   // epilogue workgroups: the epilogue kernel's shape, 128 x 512 (the upper half of such a workgroup returns at once: 64 x 1024 measured 8 us slower per iteration, as in round 5)
template <bool ODD>
__global__ void __launch_bounds__(kLatThreads, 1) vhp_planner_iteration(LatArgs<double> a, PlannerDev d) {
  extern __shared__ double lds[];
  if (blockIdx.x >= (unsigned)kUnits) {
    if (threadIdx.x < (unsigned)kEpilogueThreads)
      planner_epilogue_body<kEpilogueThreads>(a.m.nx, a.m.ny, d, (int)blockIdx.x - kUnits, (int)gridDim.x - kUnits, d.ticket + 1, (unsigned)kUnits);
    return;
  }
  const Layout L = make_layout(kLatWaves, 1, a.m.nx, a.m.ny, kLatTilePitch);
  using WorkerT = LatWorkerT<double, ODD>;
  WorkerT::clear(lds, L, (int)threadIdx.x, kLatThreads);
  __syncthreads();
  WorkerT wk;
  wk.init(a, lds, L, uniform((int)(threadIdx.x >> 6)));
  wk.run((int)blockIdx.x);
  // this octant's stores are out: counted for the epilogue's workgroups (every wavefront drains its stores, the barrier, then one
  // lane releases at agent scope -- the readers sit behind other L2s -- and counts)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!d.local_uncached) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    (void)__hip_atomic_fetch_add(d.ticket + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One thread per word of the four diagonal-packed maps (DiagMaps): its 64 cells of the byte map.  Once per vhp_set_map.
__global__ void vhp_pack_diag(const uint8_t* __restrict__ occ, uint64_t* __restrict__ dmap, int nx, int ny) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= DiagMaps::words(nx, ny)) return;
  const size_t by_y0 = DiagMaps::offset(nx, ny, 2);
  const bool by_y = k >= by_y0;
  const int wpd = by_y ? DiagMaps::wpdy(ny) : DiagMaps::wpdx(nx);
  const size_t r = by_y ? k - by_y0 : k;
  const size_t run_all = r / (size_t)wpd;
  const int word = (int)(r - run_all * (size_t)wpd), n_runs = DiagMaps::runs(nx, ny);
  const bool anti = run_all >= (size_t)n_runs;
  const int id = (int)(anti ? run_all - (size_t)n_runs : run_all);
  if (word == 0 || word == wpd - 1) return;  // (the pad words at either end of a run stay zero)
  uint64_t bits = 0;
  for (int t = 0; t < 64; ++t) {
    const int c = (word - 1) * 64 + t;  // x (by x) or y (by y)
    // main: y - x = id - (nx - 1); anti: y + x = id
    const int x = by_y ? (anti ? id - c : c - (id - (nx - 1))) : c;
    const int y = by_y ? c : (anti ? id - c : c + (id - (nx - 1)));
    if (x >= 0 && x < nx && y >= 0 && y < ny && occ[(size_t)y * nx + x]) bits |= 1ull << t;
  }
  dmap[k] = bits;
}

// The same words for every map of a stack (vhp_set_maps), from its row-packed copy: map blockIdx.y, gridDim.y, ... of n_maps; pad words
// written as zeros.  Once per stack, on the first planner batch that needs them (vhp_capi.hip).
__global__ void vhp_pack_diag_stack(const uint64_t* __restrict__ rows, uint64_t* __restrict__ dmap, int n_maps, int nx, int ny, int wpr) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t words = DiagMaps::words(nx, ny);
  if (k >= words) return;
  for (int m = (int)blockIdx.y; m < n_maps; m += (int)gridDim.y)
    dmap[(size_t)m * words + k] = diag_word_from_rows(rows + (size_t)m * ny * wpr, wpr, nx, ny, k);
}

// The units of a launch (8 per source: quadrant x {x-major, y-major}) by falling length of their march, for launches of more workgroups
// than the chip holds at once: a counting sort by steps / 8 in one workgroup (up to 1024 x kLatOrderPerThread units).  The length of a march is what an
// octant's time goes by (T / 16 + T / 64 windows); units of sources outside the grid go last.
__global__ void __launch_bounds__(1024) vhp_lat_order(const int32_t* __restrict__ src_xy, int n_src, int nx, int ny, int* __restrict__ order,
                                                      stamps::Entry* __restrict__ stamp_begin, unsigned long long stamp_tag) {
  // the launch's begin stamp, before anything else: the order kernel is part of what a launch costs
  if (stamp_begin && threadIdx.x == 0) write_stamp(stamp_begin, stamp_tag);
  __shared__ int hist[1024], start[1024];
  const int tid = (int)threadIdx.x, n_units = n_src * kUnits;
  hist[tid] = 0;
  __syncthreads();
  int bucket[kLatOrderPerThread], pos[kLatOrderPerThread];
#pragma unroll
  for (int r = 0; r < kLatOrderPerThread; ++r) {
    const int u = tid + 1024 * r;
    bucket[r] = 1023;
    pos[r] = 0;
    if (u < n_units) {
      const int s = u / kUnits, qo = u - s * kUnits, q = qo >> 1;
      const int sx = src_xy[2 * s], sy = src_xy[2 * s + 1];
      int T = 0;
      if (sx >= 0 && sy >= 0 && sx < nx && sy < ny) {
        const int dx = (q == 0 || q == 3) ? 1 : -1, dy = (q == 0 || q == 1) ? 1 : -1;   // (BandWorker::run's table of directions)
        const int ni = dx > 0 ? nx - sx : sx, nj = dy > 0 ? ny - sy : sy;
        T = (ni > 0 && nj > 0) ? ((qo & 1) == 0 ? ni : nj) : 0;
      }
      bucket[r] = 1023 - imin(T >> 3, 1023);
      pos[r] = atomicAdd(&hist[bucket[r]], 1);
    }
  }
  __syncthreads();
  // inclusive prefix sums of the 1024 buckets (Hillis-Steele on the workgroup's 1024 threads)
  start[tid] = hist[tid];
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = tid >= d ? start[tid - d] : 0;
    __syncthreads();
    start[tid] += v;
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < kLatOrderPerThread; ++r) {
    const int u = tid + 1024 * r;
    if (u < n_units) order[start[bucket[r]] - hist[bucket[r]] + pos[r]] = u;
  }
}

}  // namespace pool

namespace {
// (workgroups per unit, the LDS and whether the units are ordered first: vhp_launch_plan.hpp plan_lat)
template <typename OutT>
hipError_t launch_lat_t(const BatchArgs& a, const PlannerDev* pd = nullptr) {
  using namespace pool;
  const LatPlan p = plan_lat(a.nx, a.ny, a.n_src, a.n_cus, lat_needs_odd<OutT>(a.nx, a.field_stride, static_cast<const OutT*>(a.d_out)), a.lat_workgroups,
                             {a.d_lat_order != nullptr, a.lat.pivot_rec != nullptr, a.lat.src_index != nullptr, a.lat.slot_base != nullptr,
                              a.lat.map_idx != nullptr, pd != nullptr});
#ifdef VHP_EXP_ONE_KERNEL  // compile-time experiments only: one instantiation instead of eight
  auto k = vhp_lat_sweep<double, false, false>;
  if (p.odd || sizeof(OutT) != 8) return hipErrorInvalidValue;
#else
  auto k = p.halves > 1 ? (p.odd ? vhp_lat_sweep<OutT, true, true> : vhp_lat_sweep<OutT, false, true>)
                        : (p.odd ? vhp_lat_sweep<OutT, true, false> : vhp_lat_sweep<OutT, false, false>);
#endif
  // a stack of maps (a.lat.map_idx): the fp64 build of the kernel that reads a map per source
  auto ks = p.halves > 1 ? (p.odd ? vhp_lat_maps_sweep<true, true> : vhp_lat_maps_sweep<false, true>)
                         : (p.odd ? vhp_lat_maps_sweep<true, false> : vhp_lat_maps_sweep<false, false>);
  if (a.lat.map_idx && (sizeof(OutT) != 8 || pd)) return hipErrorInvalidValue;
  if (a.d_stamps && (a.lat.map_idx || pd)) return hipErrorInvalidValue;  // (the stack's build and the planner's iteration write no stamps)
  if (!p.ok || a.pool_epoch == 0) return hipErrorInvalidValue;
  if (a.raise_lds) {
    hipError_t e = a.raise_lds(a.lat.map_idx ? reinterpret_cast<const void*>(ks) : reinterpret_cast<const void*>(k), p.lds_bytes);
    if (e != hipSuccess) return e;
  }
#ifdef VHP_EXP_ONE_KERNEL
  LatArgs<double> g;
#else
  LatArgs<OutT> g;
#endif
  g.m = geom_map(a);
  g.src_xy = a.d_src;
#ifdef VHP_EXP_ONE_KERNEL
  g.out = static_cast<double*>(a.d_out);
#else
  g.out = static_cast<OutT*>(a.d_out);
#endif
  g.field_stride = a.field_stride;
  g.err_flag = a.d_err;
  g.lines = reinterpret_cast<vhp::lanes::Tagged*>(a.d_queue);
  g.unit_blocks = lat_unit_blocks(a.nx, a.ny);
  g.epoch = a.pool_epoch;
  g.src_index = a.lat.src_index;
  g.skip = a.lat.skip;
  g.pivot_rec = a.lat.pivot_rec;
  g.slot_base = a.lat.slot_base;
  g.run_if = a.lat.run_if;
  g.dead_cells_are_zero = a.lat.dark_unwritten;
  g.strip_times = nullptr;
  g.dmap = a.dmap;
  if (!g.dmap) return hipErrorInvalidValue;
  // Two workgroups per unit where an octant can have more bands than a workgroup has sweepers and the launch leaves the CUs for it
  // (vhp_band.hpp BandWorker: bands 8-15, 24-31, ... of an octant on the second one).
  g.n_units = a.n_src * kUnits;
  g.halves = p.halves;
#ifdef VHP_DIAG_POOLPROF
  { void* sym = nullptr; if (hipGetSymbolAddress(&sym, HIP_SYMBOL(pool::g_lat_strip_times)) == hipSuccess) g.strip_times = static_cast<unsigned long long*>(sym); }
#endif
  if (a.ev_begin) (void)hipEventRecord(a.ev_begin, a.stream);
#ifndef VHP_EXP_ONE_KERNEL
  if constexpr (sizeof(OutT) == 8) {
    if (pd) {  // the planner's iteration: the sweep's eight workgroups and the epilogue's in one launch
      auto kp = p.odd ? vhp_planner_iteration<true> : vhp_planner_iteration<false>;
      if (a.raise_lds) {
        hipError_t e2 = a.raise_lds(reinterpret_cast<const void*>(kp), p.lds_bytes);
        if (e2 != hipSuccess) return e2;
      }
      g.halves = 1;
      hipLaunchKernelGGL(kp, dim3((unsigned)(kUnits + kPlanEpiBlocks)), dim3(kLatThreads), p.lds_bytes, a.stream, g, *pd);
      const hipError_t e3 = hipGetLastError();
      if (a.ev_end) (void)hipEventRecord(a.ev_end, a.stream);
      return e3;
    }
  }
#endif
  // timed by the stamps its kernels write (lat_stamp_counts: the begin entry by the order kernel where there is one, else by every
  // workgroup of the sweep) or by the events
  const StampCounts sc = lat_stamp_counts(p, a.n_src);
  stamps::Entry* const stamp_begin = a.d_stamps && !p.use_order_kernel ? a.d_stamps : nullptr;
  stamps::Entry* const stamp_end = a.d_stamps ? a.d_stamps + sc.n_begin : nullptr;
  if (p.use_order_kernel) {
    // (a list of its own, not a corner of the scratch: nothing but tagged entries may ever be written where a later launch looks for tags)
    hipLaunchKernelGGL(pool::vhp_lat_order, dim3(1), dim3(1024), 0, a.stream, a.d_src, a.n_src, a.nx, a.ny, a.d_lat_order, a.d_stamps, a.pool_epoch);
    g.order = a.d_lat_order;
  }
  if (a.lat.map_idx) {
    if constexpr (sizeof(OutT) == 8) {
      const LatMapStack st{a.lat.map_idx, a.n_maps, (long long)a.ny * a.wpr, (long long)a.nx * a.wpc, (long long)DiagMaps::words(a.nx, a.ny)};
      hipLaunchKernelGGL(ks, dim3((unsigned)(a.n_src * kUnits * g.halves)), dim3(kLatThreads), p.lds_bytes, a.stream, g, st);
    }
  } else {
    hipLaunchKernelGGL(k, dim3((unsigned)(a.n_src * kUnits * g.halves)), dim3(kLatThreads), p.lds_bytes, a.stream, g, stamp_begin, stamp_end);
  }
  const hipError_t e = hipGetLastError();
  if (a.ev_end) (void)hipEventRecord(a.ev_end, a.stream);
  return e;
}
}  // namespace

size_t lat_scratch_bytes(int n_src, int nx, int ny) {
  return (size_t)pool::lat_unit_blocks(nx, ny) * pool::kUnits * (size_t)n_src * 64 * sizeof(vhp::lanes::Tagged);
}
size_t lat_order_bytes() { return (size_t)1024 * pool::kLatOrderPerThread * sizeof(int); }

size_t lat_diag_map_bytes(int nx, int ny) { return pool::DiagMaps::words(nx, ny) * sizeof(uint64_t); }

hipError_t lat_pack_diag_maps(const uint8_t* d_occ, int nx, int ny, uint64_t* d_dmap, hipStream_t stream) {
  const size_t words = pool::DiagMaps::words(nx, ny);
  hipLaunchKernelGGL(pool::vhp_pack_diag, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, d_occ, d_dmap, nx, ny);
  return hipGetLastError();
}

hipError_t lat_pack_diag_stack(const uint64_t* d_rows, int n_maps, int nx, int ny, int wpr, uint64_t* d_dmap, hipStream_t stream) {
  const size_t words = pool::DiagMaps::words(nx, ny);
  const unsigned gy = (unsigned)std::min(n_maps, 65535);  // (the kernel steps through more maps than that)
  hipLaunchKernelGGL(pool::vhp_pack_diag_stack, dim3((unsigned)((words + 255) / 256), gy), dim3(256), 0, stream, d_rows, d_dmap, n_maps, nx, ny, wpr);
  return hipGetLastError();
}

#ifdef VHP_DIAG_POOLPROF
extern "C" int vhp_debug_read_latprof(unsigned long long* dst, int n_words) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(pool::g_latprof), (size_t)n_words * 8);
}
extern "C" int vhp_debug_read_lat_strip_times(unsigned long long* dst, int n_words) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(pool::g_lat_strip_times), (size_t)n_words * 8);
}
#endif

hipError_t launch_lat(const BatchArgs& a) {
  if (!lat_supported(a.nx, a.ny)) return hipErrorInvalidValue;
  if (a.lat.planner_dev) {
    if (a.dtype != VHP_F64 || a.n_src != 1 || !a.lat.pivot_rec) return hipErrorInvalidValue;
    return launch_lat_t<double>(a, a.lat.planner_dev);
  }
  return a.dtype == VHP_F64 ? launch_lat_t<double>(a) : launch_lat_t<float>(a);
}

}  // namespace vhp
