// vhp_planner_batch.hip.h -- many independent planner queries on one map, their iterations in lock step (vhp_planner_solve_batch).
//
// A planner iteration of one query keeps few CUs busy: its sweep is eight workgroups of the latency sweep, its epilogue a pass over
// the grid that is a chain of memory latencies.  The queries of a batch are independent, so one iteration serves all that still run:
//   sweep    : ONE latency-sweep launch of the group's m sources -- source g is query g's current pivot, read on the device from the
//              candidate array (x < 0: the query has finished and its units do nothing: LatArgs::slot_base) -- into query g's local
//              field (fields nx * ny apart);
//   epilogue : vhp_planner_batch_epilogue, grid (blocks per query, m): blockIdx.y picks the query's own PlannerDev and the workgroup
//              runs planner_epilogue_body on its share of that query's cells; the query's last workgroup picks its next pivot as in
//              the single-query loop and also writes the query's candidate (the pivot, or x = -1 when the query is done), counting a
//              finished query into the group's done word.
// Every query has its own union, labels, pivots, control block, partials and ticket, and two local fields that take turns with the
// sweep's dark cells left unwritten, as in planner_solve.  The queries of a group start together, so launch n is iteration n of every
// query that still runs: the turn is global, and a query's last local field is the one of launch iters - 1.  Each query therefore
// computes exactly what planner_solve computes for it alone: the same sweep of the same pivot, the same epilogue body over the same
// state.
// The host enqueues kPollIterations iterations per poll of the done word (planner_poll); the batch runs as groups of at most G queries, one after the other
// (planner_batch_group_size in vhp_capi.hip).  Where even one source does not take the latency sweep, the groups are single queries and
// their sweep is the planner's front sweep (vhp_planner_sweep), one local field.
// The same loop serves a stack of maps (vhp_planner_solve_maps_batch, BatchStack): every slot also has its map index, uploaded with the
// queries; the group's sweep launch reads the group's slice of them (vhp_lat.hip vhp_lat_maps_sweep), the front sweep is launched on the
// query's own map.  The epilogue never reads the occupancy, and scale_ depends on nx, ny only: it serves both as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "vhp.h"
#include "vhp_planner.hip.h"

namespace vhp {

constexpr int kBatchMaxQueries = 64;   // queries per vhp_planner_solve_batch call
constexpr int kBatchMaxGroup = 32;     // queries per group (one latency-sweep launch)

struct BatchQuery {
  double threshold;
  int start_x, start_y, end_x, end_y;
};

// the control block of one query and its 16-byte pivot record (PlannerDev::ctl, PlannerDev::rec)
struct BatchCtl {
  PlannerCtl ctl;
  int rec[4];
};

// What the batch kernels need to build query g's PlannerDev: every array holds one slot per query of the group, `cells` (fields,
// labels), pivot_stride (pivots), kEpilogueBlocks (partials) or 2 (tickets) entries apart.
struct PlannerBatchDev {
  double* vis_global;
  double* local[2];        // the two local fields that take turns (local[1] null: one field, fully written by every sweep)
  uint32_t* label;
  int32_t* pivots;
  BatchCtl* ctl;
  PlannerKey* partial;
  unsigned int* ticket;
  const BatchQuery* query;
  int32_t* cand;           // (x, y) per query: the source of its next sweep, x = -1 once it is done
  unsigned int* n_done;    // queries of the group that are done
  size_t cells, pivot_stride;
  double scale;
  unsigned long long max_iter;
};

__host__ __device__ inline PlannerDev batch_query_dev(const PlannerBatchDev& b, int g, int parity) {
  PlannerDev d;
  const size_t f = (size_t)g * b.cells;
  d.vis_global = b.vis_global + f;
  d.vis_local = b.local[b.local[1] ? parity : 0] + f;
  d.vis_other = b.local[1] ? b.local[parity ^ 1] + f : nullptr;
  d.label = b.label + f;
  d.pivots = b.pivots + (size_t)g * b.pivot_stride;
  d.ctl = &b.ctl[g].ctl;
  d.rec = b.ctl[g].rec;
  d.partial = b.partial + (size_t)g * kEpilogueBlocks;
  d.ticket = b.ticket + 2 * g;
  d.threshold = b.query[g].threshold;
  d.scale = b.scale;
  d.end_x = b.query[g].end_x;
  d.end_y = b.query[g].end_y;
  d.max_iter = b.max_iter;
  d.local_uncached = 0;
  return d;
}

// vhp_planner_init for each of the group's n queries (thread g: query g), and its candidate: the start, or none when a negative
// threshold ends the loop before it begins.
__global__ void vhp_planner_batch_init(PlannerBatchDev b, int nx, int n) {
  const int g = (int)threadIdx.x;
  if (blockIdx.x != 0 || g >= n) return;
  const PlannerDev d = batch_query_dev(b, g, 0);
  const BatchQuery q = b.query[g];
  d.ctl->nb = 0;
  d.ctl->done = 0;
  d.ctl->status = VHP_OK;
  d.ctl->iters = 0;
  d.pivots[0] = q.start_x;  // lightSources_[0] = start; cameFrom_(start) = 0   (solver.cpp:121-122)
  d.pivots[1] = q.start_y;
  d.label[(size_t)q.start_y * nx + q.start_x] = 0;
  int done = 0;
  if (0.0 > d.threshold) {  // the loop condition of solver.cpp:127 fails on the all-zero union: lightSources_[0] = end (:141)
    d.pivots[0] = q.end_x;
    d.pivots[1] = q.end_y;
    d.ctl->done = done = 1;
  }
  *reinterpret_cast<int4*>(d.rec) = make_int4(done, 0, d.pivots[0], d.pivots[1]);
  b.cand[2 * g] = done ? -1 : q.start_x;
  b.cand[2 * g + 1] = q.start_y;
  if (done) atomicAdd(b.n_done, 1u);
}

// Step 2 of an iteration for every query of the group: workgroup (x, g) is workgroup x of gridDim.x over query g's cells.
__global__ void __launch_bounds__(kEpilogueThreads) vhp_planner_batch_epilogue(int nx, int ny, PlannerBatchDev b, int parity) {
  const int g = (int)blockIdx.y;
  if (b.cand[2 * g] < 0) return;   // (the query is done: nothing to read)
  const PlannerDev d = batch_query_dev(b, g, parity);
  if (!planner_epilogue_body<kEpilogueThreads>(nx, ny, d, (int)blockIdx.x, (int)gridDim.x, nullptr, 0u)) return;
  // (the one thread that has just picked the query's next pivot: the record it wrote says what the next sweep takes)
  const int4 r = *reinterpret_cast<const int4*>(d.rec);
  b.cand[2 * g] = r.x ? -1 : r.z;
  b.cand[2 * g + 1] = r.w;
  if (r.x) atomicAdd(b.n_done, 1u);
}

// Validation on a stack of maps: the occupancy bit of point i = (x, y, map k) of pts, from the map's row-packed words, into occ[i] --
// the 2Q cells of a batch in one launch and one copy.
__global__ void vhp_planner_batch_occupancy(const int4* __restrict__ pts, int n, const uint64_t* __restrict__ rows, long long rows_stride,
                                            int wpr, uint8_t* __restrict__ occ) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int4 p = pts[i];
  const uint64_t w = rows[(long long)p.z * rows_stride + (long long)p.y * wpr + 1 + (p.x >> 6)];
  occ[i] = (uint8_t)((w >> (p.x & 63)) & 1ull);
}

// A batch on a stack of maps of one size (vhp_set_maps): query q runs on map map_idx[q] (host, checked by the caller); map k's row-packed
// words are those of map 0 (rows) moved by k * rows_stride.
struct BatchStack {
  const int32_t* map_idx;
  const uint64_t* rows;
  long long rows_stride;
  int wpr;
};

// The memory of a BatchState (batch_free drops all of it at once: a member added here needs no other list).
struct BatchMem {
  DevBuf<double> vis_global;
  DevBuf<double> local[2];
  DevBuf<uint32_t> label;
  DevBuf<int32_t> pivots;
  DevBuf<BatchCtl> ctl;
  DevBuf<PlannerKey> partial;
  DevBuf<unsigned int> ticket;
  DevBuf<BatchQuery> query;
  DevBuf<int32_t> cand;
  DevBuf<int32_t> map_idx;               // per slot: its query's map (a batch on a stack of maps)
  DevBuf<int4> probe;                    // a batch on a stack: the 2 * kBatchMaxQueries cells of its validation, then their bits (bytes)
  DevBuf<unsigned int> n_done;           // [0]: done queries of the running group; [1]: zero (the sweep's LatArgs::slot_base)
  DevBuf<unsigned long long> came64;     // cells: the labels widened for vhp_planner_batch_results
  PinnedBuf<unsigned int> h_done;        // two copies of the done word (the host's polls)
};

// The device state of a batch: every array holds one slot per query that passed validation (results stay until the next batch or
// vhp_set_map), plus the host's view of the last batch.
struct BatchState : BatchMem {
  size_t cells = 0, slots = 0, pivot_stride = 0;   // what the arrays hold
  hipEvent_t poll_ev[2] = {nullptr, nullptr};
  // the last batch: per query its slot (-1: failed validation), its control block as the loop left it
  bool solved = false;
  bool two_fields = false;
  std::vector<int> slot_of;
  std::vector<int32_t> codes;             // per query: the validation code of one without a slot (vhp_planner_batch_paths reports it)
  std::vector<BatchCtl> h_ctl;
  int group = 0;                          // G of the last batch
  // set by the caller: the latency sweep of n sources cand[0 .. n) into fields out, out + cells, ... (LatArgs::slot_base: x < 0 sweeps
  // nothing, dark cells unwritten), source g on map map_idx[g] (device; null: one map) -- or null: the front sweep of query d on map
  // `map` (host; 0 on one map) (vhp_planner_sweep through launch_planner_kernel, shape R, W, multi)
  std::function<hipError_t(const int32_t* cand, const int32_t* map_idx, int n, double* out)> lat_sweep;
  std::function<hipError_t(const PlannerDev& d, int map)> front_sweep;
};

inline void batch_free(BatchState& s) {
  static_cast<BatchMem&>(s) = BatchMem{};
  for (auto& e : s.poll_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  s.cells = s.slots = s.pivot_stride = 0;
  s.solved = false;   // (what the last batch left is gone with it)
}

// bytes of device memory per cell and query of a batch: the union and two local fields (fp64), the labels (uint32)
constexpr size_t kBatchBytesPerCell = 28;

// Workgroups of the epilogue per query for a group of n queries: today's single-query shape up to 8 queries, then fewer, so that a
// launch stays near 1024 workgroups (blocks <= threads, the body's last workgroup merges one partial per lane: <= kEpilogueBlocks).
inline int batch_epilogue_blocks(int n) {
  const int b = 1024 / (n > 0 ? n : 1);
  return b > kEpilogueBlocks ? kEpilogueBlocks : b < 16 ? 16 : b;
}

// Q queries (field coordinates) with their thresholds: status[q] / n_pivots[q] as planner_solve would give them for query q alone.
// group: queries per group (1 .. kBatchMaxGroup; 1 where s.lat_sweep is null).  Returns VHP_OK or a call-level error.
// On one map (stack null) its occupancy is d_occ / h_occ (m: its shape); on a stack of maps of m's shape, query q's map is
// stack->map_idx[q] (d_occ, h_occ unused).
inline int planner_solve_batch(BatchState& s, const DevMap& m, const uint8_t* d_occ, const uint8_t* h_occ, hipStream_t stream,
                               hipEvent_t ev0, hipEvent_t ev1, const int32_t* queries, const double* thresholds, int n_queries,
                               uint64_t max_iter, int group, int32_t* status, uint32_t* n_pivots, std::string* msg,
                               const BatchStack* stack = nullptr) {
  const int nx = m.nx, ny = m.ny;
  const size_t cells = (size_t)nx * ny;
  s.solved = false;   // (until this batch has finished: a failed batch leaves no results)
  s.slot_of.assign(n_queries, -1);
  s.codes.assign(n_queries, VHP_OK);
  // the four validity checks of solve() per query, in the reference's order (solver.cpp:89-116); the occupancy of a device map is
  // fetched for all queries at once
  std::vector<uint8_t> occ(2 * (size_t)n_queries, 1);
  if (stack) {  // (the bits of each query's own map, gathered on the device: one launch, one copy)
    std::vector<int4> pts;
    std::vector<int> at;   // the entry of occ that point i answers
    for (int q = 0; q < n_queries; ++q) {
      const int32_t* p = queries + 4 * q;
      if (!planner_in_bounds(nx, ny, p[0], p[1]) || !planner_in_bounds(nx, ny, p[2], p[3])) continue;
      for (int e = 0; e < 2; ++e) {
        pts.push_back(make_int4(p[2 * e], p[2 * e + 1], stack->map_idx[q], 0));
        at.push_back(2 * q + e);
      }
    }
    if (!pts.empty()) {
      const int n = (int)pts.size();   // (<= 2 * kBatchMaxQueries)
      VHP_PL_HIP(s.probe.grow(2 * kBatchMaxQueries * (sizeof(int4) + 1)));
      uint8_t* d_bits = reinterpret_cast<uint8_t*>(s.probe.get() + 2 * kBatchMaxQueries);
      std::vector<uint8_t> bits(n);
      VHP_PL_HIP(hipMemcpyAsync(s.probe.get(), pts.data(), n * sizeof(int4), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(vhp_planner_batch_occupancy, dim3(1), dim3(2 * kBatchMaxQueries), 0, stream, s.probe.get(), n, stack->rows,
                         stack->rows_stride, stack->wpr, d_bits);
      VHP_PL_HIP(hipGetLastError());
      VHP_PL_HIP(hipMemcpyAsync(bits.data(), d_bits, n, hipMemcpyDeviceToHost, stream));
      VHP_PL_HIP(hipStreamSynchronize(stream));
      for (int i = 0; i < n; ++i) occ[at[i]] = bits[i];
    }
  } else if (const int rc = planner_fetch_occupancy(h_occ, d_occ, nx, ny, stream, queries, n_queries, occ.data(), msg); rc != VHP_OK) {
    return rc;
  }
  std::vector<BatchQuery> run;
  std::vector<int32_t> run_map;   // (a stack: the map of each slot)
  std::string first_msg;
  for (int q = 0; q < n_queries; ++q) {
    const int32_t* p = queries + 4 * q;
    const QueryCheck c = planner_check_query(nx, ny, p[0], p[1], p[2], p[3], occ[2 * q], occ[2 * q + 1]);
    status[q] = c.code;
    n_pivots[q] = 0;
    s.codes[q] = c.code;
    if (c.code != VHP_OK) {
      if (first_msg.empty()) first_msg = "query " + std::to_string(q) + ": " + c.msg;
      continue;
    }
    s.slot_of[q] = (int)run.size();
    run.push_back(BatchQuery{thresholds[q], p[0], p[1], p[2], p[3]});
    run_map.push_back(stack ? stack->map_idx[q] : 0);
  }
  const size_t n_run = run.size();
  const size_t pstride = planner_pivot_ints(max_iter);
  const bool two_fields = (bool)s.lat_sweep;
  if (!s.lat_sweep) group = 1;
  // (re)allocation: grow-only in queries and pivots; a new grid starts afresh
  if (s.cells != cells || s.slots < n_run || s.pivot_stride < pstride || (two_fields && !s.local[1].get() && s.slots)) {
    const size_t slots = std::max(n_run, s.cells == cells ? s.slots : (size_t)0);
    batch_free(s);
    if (slots > 0) {
      VHP_PL_HIP(s.vis_global.grow(slots * cells * 8));
      VHP_PL_HIP(s.local[0].grow(slots * cells * 8));
      if (two_fields) VHP_PL_HIP(s.local[1].grow(slots * cells * 8));
      VHP_PL_HIP(s.label.grow(slots * cells * 4));
      VHP_PL_HIP(s.pivots.grow(slots * pstride * sizeof(int32_t)));
      VHP_PL_HIP(s.ctl.grow(slots * sizeof(BatchCtl)));
      VHP_PL_HIP(s.partial.grow(slots * kEpilogueBlocks * sizeof(PlannerKey)));
      VHP_PL_HIP(s.ticket.grow(slots * 2 * sizeof(unsigned int)));
      VHP_PL_HIP(s.query.grow(slots * sizeof(BatchQuery)));
      VHP_PL_HIP(s.cand.grow(slots * 2 * sizeof(int32_t)));
      VHP_PL_HIP(s.map_idx.grow(slots * sizeof(int32_t)));
    }
    VHP_PL_HIP(s.n_done.grow(2 * sizeof(unsigned int)));
    VHP_PL_HIP(s.h_done.grow(2 * sizeof(unsigned int)));
    for (auto& e : s.poll_ev) VHP_PL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s.cells = cells;
    s.slots = slots;
    s.pivot_stride = pstride;
  }
  s.two_fields = two_fields;
  s.group = group;
  s.h_ctl.assign(n_run, BatchCtl{});
  VHP_PL_HIP(hipEventRecord(ev0, stream));
  if (n_run > 0) {
    // reset() for every query (solver.cpp:42-47)
    VHP_PL_HIP(hipMemsetAsync(s.vis_global.get(), 0, n_run * cells * 8, stream));
    VHP_PL_HIP(hipMemsetAsync(s.local[0].get(), 0, n_run * cells * 8, stream));
    if (two_fields) VHP_PL_HIP(hipMemsetAsync(s.local[1].get(), 0, n_run * cells * 8, stream));
    VHP_PL_HIP(hipMemsetAsync(s.label.get(), 0xff, n_run * cells * 4, stream));
    VHP_PL_HIP(hipMemsetAsync(s.pivots.get(), 0, n_run * s.pivot_stride * sizeof(int32_t), stream));
    VHP_PL_HIP(hipMemsetAsync(s.ticket.get(), 0, n_run * 2 * sizeof(unsigned int), stream));
    VHP_PL_HIP(hipMemcpyAsync(s.query.get(), run.data(), n_run * sizeof(BatchQuery), hipMemcpyHostToDevice, stream));
    if (stack) VHP_PL_HIP(hipMemcpyAsync(s.map_idx.get(), run_map.data(), n_run * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  VHP_PL_HIP(hipMemsetAsync(s.n_done.get(), 0, 2 * sizeof(unsigned int), stream));

  PlannerBatchDev all;
  all.vis_global = s.vis_global.get();
  all.local[0] = s.local[0].get();
  all.local[1] = two_fields ? s.local[1].get() : nullptr;
  all.label = s.label.get();
  all.pivots = s.pivots.get();
  all.ctl = s.ctl.get();
  all.partial = s.partial.get();
  all.ticket = s.ticket.get();
  all.query = s.query.get();
  all.cand = s.cand.get();
  all.n_done = s.n_done.get();
  all.cells = cells;
  all.pivot_stride = s.pivot_stride;
  all.scale = planner_scale(nx, ny);
  all.max_iter = max_iter;
  for (size_t g0 = 0; g0 < n_run; g0 += (size_t)group) {
    const int n = (int)std::min((size_t)group, n_run - g0);
    // the group's view: slot g0 + g is its query g
    PlannerBatchDev b = all;
    const size_t f = g0 * cells;
    b.vis_global += f;
    b.local[0] += f;
    if (b.local[1]) b.local[1] += f;
    b.label += f;
    b.pivots += g0 * s.pivot_stride;
    b.ctl += g0;
    b.partial += g0 * kEpilogueBlocks;
    b.ticket += 2 * g0;
    b.query += g0;
    b.cand += 2 * g0;
    VHP_PL_HIP(hipMemsetAsync(all.n_done, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(vhp_planner_batch_init, dim3(1), dim3(64), 0, stream, b, nx, n);
    VHP_PL_HIP(hipGetLastError());
    const int blocks = batch_epilogue_blocks(n);
    size_t launches = 0;
    auto enqueue = [&]() -> int {
      for (int k = 0; k < kPollIterations; ++k, ++launches) {   // (iterations past a query's end see its candidate x = -1 and return at once)
        const int parity = (int)(launches & 1);
        hipError_t e = hipSuccess;
        if (s.lat_sweep) {
          e = s.lat_sweep(b.cand, stack ? s.map_idx.get() + g0 : nullptr, n, b.local[parity]);
        } else {
          e = s.front_sweep(batch_query_dev(b, 0, 0), run_map[g0]);
        }
        if (e != hipSuccess) { *msg = std::string("batch planner launch: ") + hipGetErrorString(e); return VHP_ERR_HIP; }
        hipLaunchKernelGGL(vhp_planner_batch_epilogue, dim3(blocks, n), dim3(kEpilogueThreads), 0, stream, nx, ny, b, parity);
        VHP_PL_HIP(hipGetLastError());
      }
      return VHP_OK;
    };
    // (the group's loop ends when the done word counts all its queries)
    unsigned int n_done = 0;
    const int rc = planner_poll(stream, all.n_done, s.h_done.get(), s.poll_ev, enqueue, [n](unsigned int done) { return done >= (unsigned)n; },
                                "batch planner poll", &n_done, msg);
    if (rc != VHP_OK) return rc;
  }
  VHP_PL_HIP(hipEventRecord(ev1, stream));
  if (n_run > 0) VHP_PL_HIP(hipMemcpyAsync(s.h_ctl.data(), all.ctl, n_run * sizeof(BatchCtl), hipMemcpyDeviceToHost, stream));
  VHP_PL_HIP(hipStreamSynchronize(stream));
  for (int q = 0; q < n_queries; ++q) {
    if (s.slot_of[q] < 0) continue;
    const PlannerCtl& c = s.h_ctl[s.slot_of[q]].ctl;
    status[q] = c.status;
    n_pivots[q] = (uint32_t)c.nb;
  }
  s.solved = true;
  *msg = first_msg;
  return VHP_OK;
}

// The device arrays of query slot k of the last batch (the local field: the one its last iteration swept into).
inline void batch_results_device(const BatchState& s, int k, const uint32_t** labels, const double** vis_global, const double** vis_local,
                                 const int32_t** pivots_xy) {
  const size_t f = (size_t)k * s.cells;
  const int iters = s.h_ctl[k].ctl.iters;
  const int which = (s.two_fields && iters > 0 && ((iters - 1) & 1)) ? 1 : 0;
  if (labels) *labels = s.label.get() + f;
  if (vis_global) *vis_global = s.vis_global.get() + f;
  if (vis_local) *vis_local = s.local[which].get() + f;
  if (pivots_xy) *pivots_xy = s.pivots.get() + (size_t)k * s.pivot_stride;
}

// Host copies of query slot k's results, laid out as planner_solve's outputs (any may be null).
inline int batch_results_host(BatchState& s, int k, hipStream_t stream, uint64_t* came_from, double* vis_global, double* vis_local,
                              int32_t* pivots_xy, std::string* msg) {
  const uint32_t* lab;
  const double *vg, *vl;
  const int32_t* piv;
  batch_results_device(s, k, &lab, &vg, &vl, &piv);
  if (came_from) VHP_PL_HIP(s.came64.grow(s.cells * 8));
  return planner_copy_out(stream, s.cells, lab, s.came64.get(), vg, vl, piv, (uint32_t)s.h_ctl[k].ctl.nb, came_from, vis_global, vis_local, pivots_xy, msg,
                          true);
}

}  // namespace vhp
