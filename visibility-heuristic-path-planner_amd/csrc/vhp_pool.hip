// vhp_pool.hip -- gfx950 build of the pool sweep (vhp_pool.hpp), its unit-order pre-kernel and its launcher.
#include "vhp_batch_launch.h"

#include <hip/hip_runtime.h>

#include "vhp.h"
#include "vhp_pool.hpp"
#include "vhp_pool_scratch.hpp"

namespace vhp {
namespace pool {

// One persistent workgroup per CU; every wavefront is a Worker (kWaves, kWavesAny: vhp_launch_plan.hpp).
// A launch's timestamp (vhp_stamps.hpp): the device's constant-rate clock and the launch's tag, one 16-byte store by the calling lane.
__device__ __forceinline__ void write_stamp(stamps::Entry* p, unsigned long long tag) {
  *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2((unsigned long long)wall_clock64(), tag);
}

// stamp_end (or null: nothing is written): where workgroup g leaves the launch's end stamp [g] once all its wavefronts are done
template <typename OutT, bool ANYW>
__global__ void __launch_bounds__(64 * kWaves, 1) vhp_pool_sweep(Args<OutT> a, int n_ctx, stamps::Entry* __restrict__ stamp_end) {
  extern __shared__ double lds[];
  constexpr int W = ANYW ? kWavesAny : kWaves;
  const Layout L = make_layout(W, n_ctx, a.m.nx, a.m.ny, ANYW ? kTStrideAny : kTStride);
  Worker<OutT, ANYW>::clear(lds, L, (int)threadIdx.x, 64 * W);
  __syncthreads();
  Worker<OutT, ANYW> wk;
  wk.init(a, lds, L, uniform((int)(threadIdx.x >> 6)), (int)blockIdx.x);
  wk.run();
  if (stamp_end) {  // (a workgroup that found no unit stamps as well: the host expects every entry)
    // the wavefronts leave run() at different times: each waits for its own stores, the barrier, then one lane reads the clock
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) write_stamp(stamp_end + blockIdx.x, a.epoch);
  }
}

// Launch order: one workgroup counting-sorts the 8 n_src units by the length of their march (then by cell count), longest first,
// sets the pull queue to where the launch starts pulling (queue0: 0, or behind the units that the contexts take by workgroup
// index, Args::static_round), lays the units' boundary lines out in the scratch (first 64-entry block of unit u: exclusive prefix
// sum of UnitGeo::line_blocks in unit order) and writes the launch's records: recs[k] = {unit, sx | sy << 16, line base, 0} of the
// k-th unit in launch order.  Units of out-of-range sources weigh nothing, sort last and carry -1 in place of the source (they
// are rejected when they are installed).  If the lines do not fit `capacity_blocks` (the launcher sizes the scratch by an upper
// bound, so they do) nothing is swept and the error flag says so.
constexpr int kOrderLdsUnits = 8192;  // batches of up to 1024 sources are ordered in LDS alone (order_units_lds)

// exclusive prefix sums over arr[0..n), in place, by the 1024 threads of the workgroup (a contiguous chunk each); returns the total
template <typename Arr>
__device__ __forceinline__ int block_exclusive_scan_1024(Arr arr, int n, int* wave_tot) {
  const int per = (n + 1023) / 1024;
  const int lo = (int)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  int mine = 0;
  for (int k = lo; k < hi; ++k) mine += arr[k];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_tot[wv] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { before += k < wv ? wave_tot[k] : 0; all += wave_tot[k]; }
  int at = before + inc - mine;
  for (int k = lo; k < hi; ++k) { const int v = arr[k]; arr[k] = at; at += v; }
  __syncthreads();
  return all;
}

// (batches of more than kOrderLdsUnits units; PerUnit: line_base itself, in global memory)
template <typename PerUnit>
__device__ __forceinline__ void order_units(const int32_t* __restrict__ src_xy, int n_src, int nx, int ny, int* __restrict__ order,
                                            int* __restrict__ line_base, int* __restrict__ recs, long long capacity_blocks,
                                            unsigned long long* __restrict__ queue, unsigned long long queue0,
                                            int* __restrict__ err_flag, int* hist, int* wave_tot, PerUnit blocks) {
  const int n_units = n_src * kUnits;
  const double inv_area = 1.0 / ((double)nx * (double)ny), inv_side = 1.0 / (double)(nx > ny ? nx : ny);
  hist[threadIdx.x] = 0;
  __syncthreads();
  // one pass over the units: the blocks of a unit's boundary lines and its bucket (0 = first), kept for the two scatters below
  for (int u = threadIdx.x; u < n_units; u += 1024) {
    const int s = u / kUnits, qo = u - s * kUnits;
    const int sx = src_xy[2 * s], sy = src_xy[2 * s + 1];
    int nb = 0, bucket = kBuckets - 1;
    if (!(sx < 0 || sy < 0 || sx >= nx || sy >= ny)) {
      UnitGeo g;
      g.init(nx, ny, qo, sx, sy);
      nb = g.line_blocks();
      bucket = unit_launch_bucket(g, inv_area, inv_side);
    }
    blocks[u] = nb | (bucket << 20);  // (nb < 2^20: a unit has at most 129 strips of 130 blocks)
    atomicAdd(&hist[bucket], 1);
  }
  __syncthreads();
  (void)block_exclusive_scan_1024(hist, kBuckets, wave_tot);
  for (int u = threadIdx.x; u < n_units; u += 1024) order[atomicAdd(&hist[blocks[u] >> 20], 1)] = u;
  __syncthreads();
  for (int u = threadIdx.x; u < n_units; u += 1024) blocks[u] &= (1 << 20) - 1;
  __syncthreads();
  const int total = block_exclusive_scan_1024(blocks, n_units, wave_tot);
  const bool fits = (long long)total <= capacity_blocks;
  // the records, in launch order (order[] was written by this workgroup before the barriers above).  If the boundary lines do not fit
  // the scratch, NOTHING is swept: the queue starts exhausted, and every record says so as well (-2) -- the first unit of a context is
  // handed out by workgroup index without a look at the queue (Args::static_round), and its lines would lie beyond the scratch.
  for (int k = threadIdx.x; k < n_units; k += 1024) {
    const int u = order[k], s = u / kUnits;
    const int sx = src_xy[2 * s], sy = src_xy[2 * s + 1];
    const bool inside = !(sx < 0 || sy < 0 || sx >= nx || sy >= ny);
    reinterpret_cast<int4*>(recs)[k] = make_int4(u, !fits ? -2 : inside ? (sx | (sy << 16)) : -1, blocks[u], 0);
  }
  if (threadIdx.x == 0) {
    *queue = fits ? queue0 : (unsigned long long)n_units;
    if (!fits) atomicOr(err_flag, 4);
  }
}

// The same ordering for batches of up to kOrderLdsUnits units (1024 sources), without a round trip through global memory: every thread
// owns a contiguous chunk of at most 8 units from the first pass to the last, so a unit's line blocks and bucket (unit_key, read back
// by the thread that wrote them) and its source (src_key, written by the owner of the source's first unit, read behind a barrier) stay
// in LDS, the histogram's scan and the scan of the line blocks -- which runs in unit order and does not wait for the sort -- share one
// pass and one barrier, and a unit's record goes straight to the slot its bucket hands out: order[] and line_base[] are not written
// (nothing but the other path reads them).  Same buckets, same line bases, same queue word and error flag as order_units; units of one
// bucket follow each other as the LDS atomics retire, there as here.
__device__ __forceinline__ void order_units_lds(const int32_t* __restrict__ src_xy, int n_src, int nx, int ny, int* __restrict__ recs,
                                                long long capacity_blocks, unsigned long long* __restrict__ queue, unsigned long long queue0,
                                                int* __restrict__ err_flag, int* hist, int* wave_tot, int* unit_key, int* src_key) {
  const int n_units = n_src * kUnits;
  const int per = (n_units + 1023) / 1024;
  const int lo = (int)threadIdx.x * per, hi = lo + per < n_units ? lo + per : n_units;
  const double inv_area = 1.0 / ((double)nx * (double)ny), inv_side = 1.0 / (double)(nx > ny ? nx : ny);
  hist[threadIdx.x] = 0;
  __syncthreads();
  int mine = 0;
  for (int u = lo; u < hi; ++u) {
    const int s = u / kUnits, qo = u - s * kUnits;
    const int sx = src_xy[2 * s], sy = src_xy[2 * s + 1];
    const bool inside = !(sx < 0 || sy < 0 || sx >= nx || sy >= ny);
    int nb = 0, bucket = kBuckets - 1;
    if (inside) {
      UnitGeo g;
      g.init(nx, ny, qo, sx, sy);
      nb = g.line_blocks();
      bucket = unit_launch_bucket(g, inv_area, inv_side);
    }
    unit_key[u] = nb | (bucket << 20);
    if (qo == 0) src_key[s] = inside ? (sx | (sy << 16)) : -1;
    mine += nb;
    atomicAdd(&hist[bucket], 1);
  }
  __syncthreads();
  // two exclusive scans off one pass: the buckets' counts (one per thread) and the chunks' line blocks
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int count = hist[threadIdx.x];
  int inc_h = count, inc_b = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int th = __shfl_up(inc_h, off, 64), tb = __shfl_up(inc_b, off, 64);
    if (lane >= off) { inc_h += th; inc_b += tb; }
  }
  if (lane == 63) { wave_tot[wv] = inc_h; wave_tot[16 + wv] = inc_b; }
  __syncthreads();
  int before_h = 0, before_b = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    before_h += k < wv ? wave_tot[k] : 0;
    before_b += k < wv ? wave_tot[16 + k] : 0;
    total += wave_tot[16 + k];
  }
  hist[threadIdx.x] = before_h + inc_h - count;  // (its own entry, which no other thread has read since the barrier before the scan)
  __syncthreads();
  const bool fits = (long long)total <= capacity_blocks;
  // the records (see order_units for what they say when the lines do not fit)
  int at = before_b + inc_b - mine;
  for (int u = lo; u < hi; ++u) {
    const int key = unit_key[u], nb = key & ((1 << 20) - 1);
    const int k = atomicAdd(&hist[key >> 20], 1);
    reinterpret_cast<int4*>(recs)[k] = make_int4(u, !fits ? -2 : src_key[u / kUnits], at, 0);
    at += nb;
  }
  if (threadIdx.x == 0) {
    *queue = fits ? queue0 : (unsigned long long)n_units;
    if (!fits) atomicOr(err_flag, 4);
  }
}

__global__ void __launch_bounds__(1024) vhp_pool_order(const int32_t* __restrict__ src_xy, int n_src, int nx, int ny, int* __restrict__ order,
                                                       int* __restrict__ line_base, int* __restrict__ recs, long long capacity_blocks,
                                                       unsigned long long* __restrict__ queue, unsigned long long queue0,
                                                       int* __restrict__ err_flag, stamps::Entry* __restrict__ stamp_begin,
                                                       unsigned long long stamp_tag) {
  // the launch's begin stamp, before anything else: the order kernel is part of what a launch costs
  if (stamp_begin && threadIdx.x == 0) write_stamp(stamp_begin, stamp_tag);
  __shared__ int hist[kBuckets];
  __shared__ int wave_tot[32];
  __shared__ int blocks[kOrderLdsUnits];
  __shared__ int src_key[kOrderLdsUnits / kUnits];
  VHP_DIAG_TL_RESET
  if (n_src * kUnits <= kOrderLdsUnits) order_units_lds(src_xy, n_src, nx, ny, recs, capacity_blocks, queue, queue0, err_flag, hist, wave_tot, blocks, src_key);
  else order_units(src_xy, n_src, nx, ny, order, line_base, recs, capacity_blocks, queue, queue0, err_flag, hist, wave_tot, line_base);
}

}  // namespace pool

namespace {
// (what a launch decides -- contexts, heads, the first round: vhp_launch_plan.hpp; the sizes of its scratch: vhp_pool_scratch.hpp)
template <typename OutT>
hipError_t launch_pool_t(const BatchArgs& a) {
  using namespace pool;
  const bool anyw = pool_needs_anyw<OutT>(a.nx, a.field_stride > 0 ? a.field_stride : (long long)a.nx * a.ny, static_cast<const OutT*>(a.d_out));
  auto k = anyw ? vhp_pool_sweep<OutT, true> : vhp_pool_sweep<OutT, false>;
  const PoolPlan p = plan_pool(a.nx, a.ny, a.n_src, a.n_cus, anyw, a.pool);
  if (!p.ok || a.pool_epoch == 0) return hipErrorInvalidValue;
  if (a.raise_lds) {
    hipError_t e = a.raise_lds(reinterpret_cast<const void*>(k), p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  char* scratch = reinterpret_cast<char*>(a.d_queue);
  Args<OutT> g;
  g.m = geom_map(a);
  g.out = static_cast<OutT*>(a.d_out);
  g.field_stride = a.field_stride;
  g.err_flag = a.d_err;
  g.queue = reinterpret_cast<unsigned long long*>(a.d_queue);
  g.n_units = a.n_src * kUnits;
  int* recs = a.d_queue + kQueueInts;  // (16-byte aligned: the scratch is, and kQueueInts is a multiple of 4)
  int* order = recs + 4 * (size_t)g.n_units;
  int* line_base = order + g.n_units;
  g.recs = recs;
  g.diag = reinterpret_cast<double*>(scratch + head_bytes(a.n_src));
  g.diag_stride = diag_stride_of(a.nx, a.ny);
  g.lines = reinterpret_cast<vhp::lanes::Tagged*>(scratch + head_bytes(a.n_src) + diag_bytes(a.n_src, a.nx, a.ny));
  g.epoch = a.pool_epoch;
  g.busy_cap = p.busy_cap;
  g.n_head = p.n_head;
  g.tail_limit = p.tail_limit;
  g.early_ctx = p.early_ctx;
  g.late_after = p.late_after;
  g.claim_ahead = p.claim_ahead;
  g.n_groups = a.n_cus;
  g.static_snake = p.static_snake;
  g.static_round = p.static_round;
  // timed by the stamps its kernels write (one begin entry, then one end entry per workgroup: pool_stamp_counts) or by the events
  stamps::Entry* const stamp_end = a.d_stamps ? a.d_stamps + pool_stamp_counts(a.n_cus).n_begin : nullptr;
  if (a.ev_begin) (void)hipEventRecord(a.ev_begin, a.stream);  // the order pre-kernel is part of what a launch costs
  hipLaunchKernelGGL(vhp_pool_order, dim3(1), dim3(1024), 0, a.stream, a.d_src, a.n_src, a.nx, a.ny, order, line_base, recs,
                     line_blocks_per_source(a.nx, a.ny) * a.n_src, reinterpret_cast<unsigned long long*>(a.d_queue), p.queue0, a.d_err,
                     a.d_stamps, a.pool_epoch);
  hipLaunchKernelGGL(k, dim3((unsigned)a.n_cus), dim3(64 * p.waves), p.lds_bytes, a.stream, g, p.n_ctx, stamp_end);
  const hipError_t e = hipGetLastError();
  if (a.ev_end) (void)hipEventRecord(a.ev_end, a.stream);
  return e;
}
}  // namespace

size_t pool_scratch_bytes(int n_src, int nx, int ny) {
  return head_bytes(n_src) + diag_bytes(n_src, nx, ny) + (size_t)line_blocks_per_source(nx, ny) * (size_t)n_src * 64 * sizeof(vhp::lanes::Tagged);
}

#ifdef VHP_DIAG_TIMELINE
extern "C" int vhp_debug_read_hist(unsigned long long* dst, int n_words) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(pool::g_pp_hist), (size_t)n_words * 8);
}
extern "C" int vhp_debug_read_units(unsigned* dst, int n_words) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(pool::g_pp_unit), (size_t)n_words * 4);
}
#endif

hipError_t launch_pool(const BatchArgs& a) {
  if (!pool_supported(a.nx, a.ny)) return hipErrorInvalidValue;
  return a.dtype == VHP_F64 ? launch_pool_t<double>(a) : launch_pool_t<float>(a);
}

}  // namespace vhp
