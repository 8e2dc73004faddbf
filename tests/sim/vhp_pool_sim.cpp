// vhp_pool_sim.cpp -- CPU simulator of the pool sweep kernel.  TEST INFRASTRUCTURE ONLY.
//
// Compiles csrc/vhp_pool.hpp -- the very source hipcc builds for gfx950 -- with -DVHP_SIM, where a wavefront's lane
// vector is an array of 64 values (csrc/vhp_lanes.hpp).  The kernel is blocking code (a wavefront that has to wait loops
// over backoff()), so every wavefront runs as a coroutine (ucontext) on a stack of its own: backoff() switches to the
// scheduler below, which picks the next wavefront under one of several policies, and the places where a device
// wavefront can be overtaken between a read and the compare-and-swap that depends on it (sim_point) switch too, always or
// at random.  G workgroups of W wavefronts share the unit queue, each workgroup with its own NaN-poisoned LDS; the
// diagonal scratch lines start as NaN as well.  Every interleaving must give the oracle's bytes; when every wavefront
// has waited many times in a row without any of them getting anything done the run is reported as a deadlock.
//
// Only tests/ loads this library (tests/sim_lib.py).  It is not a CPU fallback of the product: libvhp_hip.so neither
// links nor loads it.
#define VHP_SIM
#include <ucontext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../visibility-heuristic-path-planner_amd/csrc/vhp_launch_plan.hpp"
#include "../../visibility-heuristic-path-planner_amd/csrc/vhp_pool_scratch.hpp"

using namespace vhp::pool;

namespace {

struct HostMap {
  std::vector<uint64_t> rows, cols, diag;
  std::vector<double> recip;
  Map m;
};

// the packed maps and the reciprocal table, as vhp_set_map builds them (vhp_capi.hip finish_set_map)
void build_map(const uint8_t* occ, int nx, int ny, HostMap& h) {
  const int wpr = (nx + 63) / 64 + 2, wpc = (ny + 63) / 64 + 2;
  h.rows.assign((size_t)ny * wpr, 0);
  h.cols.assign((size_t)nx * wpc, 0);
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x)
      if (occ[(size_t)y * nx + x]) {
        h.rows[(size_t)y * wpr + 1 + (x >> 6)] |= 1ull << (x & 63);
        h.cols[(size_t)x * wpc + 1 + (y >> 6)] |= 1ull << (y & 63);
      }
  // the grid packed along its diagonals (vhp_band.hpp DiagMaps; vhp_capi.hip vhp_pack_diag)
  h.diag.assign(DiagMaps::words(nx, ny), 0);
  {
    const int wx = DiagMaps::wpdx(nx), wy = DiagMaps::wpdy(ny);
    uint64_t* mx = h.diag.data() + DiagMaps::offset(nx, ny, 0);
    uint64_t* ax = h.diag.data() + DiagMaps::offset(nx, ny, 1);
    uint64_t* my = h.diag.data() + DiagMaps::offset(nx, ny, 2);
    uint64_t* ay = h.diag.data() + DiagMaps::offset(nx, ny, 3);
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x)
        if (occ[(size_t)y * nx + x]) {
          const size_t im = (size_t)(y - x + nx - 1), ia = (size_t)(y + x);
          mx[im * wx + 1 + (x >> 6)] |= 1ull << (x & 63);
          ax[ia * wx + 1 + (x >> 6)] |= 1ull << (x & 63);
          my[im * wy + 1 + (y >> 6)] |= 1ull << (y & 63);
          ay[ia * wy + 1 + (y >> 6)] |= 1ull << (y & 63);
        }
  }
  const int nrec = (nx > ny ? nx : ny) + 1 + 8;
  h.recip.resize(nrec);
  h.recip[0] = 0.0;
  for (int k = 1; k < nrec; ++k) {
    volatile double d = (double)k;
    h.recip[k] = 1.0 / d;
  }
  h.m.rows = h.rows.data();
  h.m.cols = h.cols.data();
  h.m.recip = h.recip.data();
  h.m.wpr = wpr;
  h.m.wpc = wpc;
  h.m.nx = nx;
  h.m.ny = ny;
}

// ---- coroutines ----------------------------------------------------------------------------------------------------
struct Coro {
  ucontext_t ctx;
  std::unique_ptr<char[]> stack;
  bool done = false;
  void (*entry)(void*) = nullptr;
  void* arg = nullptr;
};
constexpr size_t kStack = 2u << 20;
ucontext_t g_sched;
Coro* g_cur = nullptr;
long long g_progress = 0, g_switches = 0;
int g_point_mode = 0;  // 0: points never switch, 1: always, 2: at random
uint32_t g_rng = 1;

uint32_t lcg() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
void do_yield() { ++g_switches; swapcontext(&g_cur->ctx, &g_sched); }
void hook_yield() { do_yield(); }
void hook_progress() { ++g_progress; }
void hook_point() { if (g_point_mode == 1 || (g_point_mode == 2 && (lcg() & 1))) do_yield(); }
void trampoline() {
  g_cur->entry(g_cur->arg);
  g_cur->done = true;
  swapcontext(&g_cur->ctx, &g_sched);
}

template <typename OutT, bool ANYW>
void worker_entry(void* p) { static_cast<Worker<OutT, ANYW>*>(p)->run(); }

// policy & 7: 0 round robin, 1 backward, 2 random wavefront, 3 greedy (the same wavefront again while it gets things done),
// 4 random with bursts;  policy & 8: sim points always switch;  policy & 16: sim points switch at random
template <typename OutT, bool ANYW>
int run_batch_t(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, OutT* out, int W, int C, int G, int policy,
              uint32_t seed, long long* stats) {
  HostMap h;
  build_map(occ, nx, ny, h);
  const Layout L = make_layout(W, C, nx, ny, ANYW ? kTStrideAny : kTStride);
  const int n_units = n_src * kUnits;
  // launch order: by cell count, largest first -- the simulator's own order, not vhp_pool_order's (that one goes by the length of the
  // march, unit_launch_bucket); policy & 32: shuffled instead -- the result must not depend on the order
  std::vector<int> order(n_units), line_base(n_units, 0);
  std::vector<double> weight(n_units, -1.0);
  long long line_blocks = 0;
  for (int u = 0; u < n_units; ++u) {
    order[u] = u;
    line_base[u] = (int)line_blocks;
    const int s = u / kUnits, qo = u % kUnits, sx = src[2 * s], sy = src[2 * s + 1];
    if (sx < 0 || sy < 0 || sx >= nx || sy >= ny) continue;
    UnitGeo g;
    g.init(nx, ny, qo, sx, sy);
    line_blocks += g.line_blocks();
    if (g.n_strips > 0) weight[u] = g.x_major ? (double)g.rows_total * g.ni - 0.5 * g.rows_total * (g.rows_total - 1.0)
                                              : (double)g.cols_total * (g.nj - 1) - 0.5 * g.cols_total * (g.cols_total - 1.0);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight[a] > weight[b]; });
  g_rng = seed * 2654435761u + 12345u;
  if (policy & 32) for (int k = n_units - 1; k > 0; --k) std::swap(order[k], order[lcg() % (k + 1)]);
  // the launch's records, as vhp_pool_order writes them: {unit, sx | sy << 16 (-1: outside the grid), line base, 0} in launch order
  std::vector<int> recs((size_t)4 * n_units + 4);
  for (int k = 0; k < n_units; ++k) {
    const int u = order[k], s = u / kUnits, sx = src[2 * s], sy = src[2 * s + 1];
    const bool inside = !(sx < 0 || sy < 0 || sx >= nx || sy >= ny);
    recs[4 * k] = u; recs[4 * k + 1] = inside ? (sx | (sy << 16)) : -1; recs[4 * k + 2] = line_base[u]; recs[4 * k + 3] = 0;
  }
  unsigned long long queue = 0;
  int err = 0;
  const int dstride = vhp::diag_stride_of(nx, ny);
  std::vector<double> diag((size_t)n_src * 4 * dstride, std::numeric_limits<double>::quiet_NaN());
  Args<OutT> a;
  a.m = h.m;
  a.out = out;
  a.field_stride = (long long)nx * ny;
  a.err_flag = &err;
  a.recs = recs.data();
  a.queue = &queue;
  a.n_units = n_units;
  a.diag = diag.data();
  a.diag_stride = dstride;
  // The boundary lines start with entries of an EARLIER launch (same values poisoned, tag epoch - 1) and, here and there,
  // with a tag from the future of the same scratch region laid out differently: only this launch's tag may be taken.
  const uint64_t epoch = 0x5A17000000000000ull + 7 + seed;
  std::vector<vhp::lanes::Tagged> lines((size_t)line_blocks * 64 + 64);
  for (size_t k = 0; k < lines.size(); ++k) { lines[k].v = std::numeric_limits<double>::quiet_NaN(); lines[k].tag = (k % 5 == 0) ? 0 : epoch - 1 - (k % 3); }
  a.lines = lines.data();
  a.epoch = epoch;
  a.n_head = std::min(1 + (int)(seed % 3), C);
  a.tail_limit = (int)((long long)n_units * (10 + (seed * 37) % 91) / 100);
  a.early_ctx = (seed & 1) ? C : 1 + (int)(seed % (unsigned)C);   // sometimes the contexts past the first few open late
  a.late_after = n_units / 2;  // one to three contexts pull from the head of the queue
  a.claim_ahead = (int)((seed * 7) % 5) * 8;   // 0, 8 .. 32 steps: a strip claimed before the strip below has reached its first window
  a.busy_cap = (policy & 64) ? 2 : W;   // policy & 64: a tight cap on the wavefronts that may sweep while units are installed
  // the first unit of every context by workgroup index wherever the launcher would do so (vhp_launch_plan.hpp plan_pool), in two runs of three
  a.n_groups = G;
  a.static_round = vhp::pool_static_round_ok((seed % 3) != 2, a.early_ctx, C, n_units, G);
  a.static_snake = (seed & 2) != 0;
  if (a.static_round) queue = vhp::pool_queue0(a.n_head, C, G);

  std::vector<std::vector<double>> lds(G, std::vector<double>(L.total, std::numeric_limits<double>::quiet_NaN()));
  std::vector<Worker<OutT, ANYW>> workers((size_t)G * W);
  std::vector<Coro> coros((size_t)G * W);
  for (int gI = 0; gI < G; ++gI) {
    Worker<OutT, ANYW>::clear(lds[gI].data(), L, 0, 1);
    for (int w = 0; w < W; ++w) {
      Worker<OutT, ANYW>& wk = workers[(size_t)gI * W + w];
      wk.init(a, lds[gI].data(), L, w, gI);
      Coro& c = coros[(size_t)gI * W + w];
      c.stack.reset(new char[kStack]);
      c.entry = worker_entry<OutT, ANYW>;
      c.arg = &wk;
      getcontext(&c.ctx);
      c.ctx.uc_stack.ss_sp = c.stack.get();
      c.ctx.uc_stack.ss_size = kStack;
      c.ctx.uc_link = nullptr;
      makecontext(&c.ctx, trampoline, 0);
    }
  }
  vhp::lanes::sim_hooks().yield = hook_yield;
  vhp::lanes::sim_hooks().progress = hook_progress;
  vhp::lanes::sim_hooks().point = hook_point;
  vhp::lanes::store_stats() = vhp::lanes::StoreStats();
  vhp::lanes::store_stats().base = reinterpret_cast<const char*>(out);
  vhp::lanes::store_stats().bytes = (size_t)n_src * nx * ny * sizeof(OutT);
  vhp::lanes::sim_counts() = vhp::lanes::SimCounts();
  g_point_mode = (policy & 8) ? 1 : (policy & 16) ? 2 : 0;
  g_progress = g_switches = 0;
  const int n = G * W, mode = policy & 7;
  int cur = mode == 1 ? n - 1 : 0, alive = n, burst = 0;
  long long last_progress = 0, stale = 0, deadlock = 0;
  while (alive > 0) {
    // pick
    if (mode == 0) cur = (cur + 1) % n;
    else if (mode == 1) cur = (cur + n - 1) % n;
    else if (mode == 2) cur = (int)(lcg() % n);
    else if (mode == 3) { if (g_progress == last_progress) cur = (cur + 1) % n; }   // greedy: stay while it gets things done
    else { if (burst-- <= 0) { cur = (int)(lcg() % n); burst = (int)(lcg() % 6); } }
    int tries = 0;
    while (coros[cur].done && tries++ < n) cur = mode == 1 ? (cur + n - 1) % n : (cur + 1) % n;  // (wavefronts that have returned are skipped in the policy's direction)
    if (coros[cur].done) break;
    last_progress = g_progress;
    g_cur = &coros[cur];
    swapcontext(&g_sched, &g_cur->ctx);
    if (coros[cur].done) --alive;
    if (g_progress == last_progress) { if (++stale > 4000LL * n) { deadlock = 1; break; } } else stale = 0;
  }
  vhp::lanes::sim_hooks() = vhp::lanes::SimHooks();
  if (deadlock && getenv("VHP_SIM_DUMP")) {  // the scheduler words of every workgroup, for debugging a stuck protocol
    for (int gI = 0; gI < G; ++gI) {
      Shared sh;
      sh.lds = lds[gI].data();
      sh.L = L;
      const int* sc = sh.sched();
      fprintf(stderr, "wg %d: queue_empty %d seq %d (queue %llu of %d)\n", gI, sc[kQEmpty], sc[kSeq], queue, n_units);
      for (int c = 0; c < C; ++c) {
        const int* cx = sh.ctx(c);
        fprintf(stderr, "  ctx %d: state %d word %x unit %d (qo %d) strips %d left %d sx %d sy %d diag %d\n   prog:", c, cx[kState], cx[kWord], cx[kUnit],
                cx[kUnit] & 7, cx[kNStrips], cx[kLeft], cx[kSxSy] & 0xffff, cx[kSxSy] >> 16, cx[kDiagReady]);
        for (int p = 0; p < cx[kNStrips] && p < L.S; ++p) fprintf(stderr, " %d", sh.prog(c)[p]);
        fprintf(stderr, "\n");
      }
    }
  }
  if (stats) {
    stats[0] = g_switches;
    stats[1] = g_progress;
    stats[2] = deadlock;
    stats[3] = vhp::lanes::store_stats().n16;
    stats[4] = vhp::lanes::store_stats().n8;
    stats[5] = err;
    stats[6] = (long long)((queue & 0xffffffffull) + (queue >> 32));
    for (int k = 0; k < 4; ++k) stats[7 + k] = vhp::lanes::sim_counts().c[k];  // hand-offs: from the ring, from global memory, "too far ahead", "overwritten while copying"
    stats[11] = vhp::lanes::store_stats().lines_whole;
    stats[12] = vhp::lanes::store_stats().lines_part;
    stats[13] = a.static_round ? 1 : 0;  // the contexts' first units were handed out by workgroup index
  }
  if (vhp::lanes::store_stats().misaligned) return 3;  // a pair stored off the grid of its own size
  return 0;
}

// (the ANYW build of the kernel where the launch needs it, as launch_pool_t picks it: vhp_pool.hip)
template <typename OutT>
int run_batch(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, OutT* out, int W, int C, int G, int policy, uint32_t seed, long long* stats) {
  return pool_needs_anyw<OutT>(nx, (long long)nx * ny, out) ? run_batch_t<OutT, true>(occ, nx, ny, src, n_src, out, W, C, G, policy, seed, stats)
                                                            : run_batch_t<OutT, false>(occ, nx, ny, src, n_src, out, W, C, G, policy, seed, stats);
}

// ---- the latency sweep (csrc/vhp_lat.hpp): one workgroup of W wavefronts per unit, strips bound to wavefronts ---------------
template <typename WorkerT>
struct LatCo {
  WorkerT wk;
  int unit;
};
template <typename WorkerT>
void lat_entry(void* p) { auto* c = static_cast<LatCo<WorkerT>*>(p); c->wk.run(c->unit); }

int g_lat_halves = 1;   // workgroups per unit of the band sweep (vhp_sim_set_lat_halves)

template <typename OutT, bool ODD, typename WorkerT>
int run_lat_t(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, OutT* out, int W, int policy, uint32_t seed, long long* stats) {
  HostMap h;
  build_map(occ, nx, ny, h);
  const Layout L = make_layout(W, 1, nx, ny, WorkerT::kTilePitch);
  const int H = (WorkerT::kRoles == 2 && g_lat_halves > 1) ? g_lat_halves : 1;   // (the sweep in strips knows no halves)
  const int n_units = n_src * kUnits;
  const int G = n_units * H;   // workgroups
  int err = 0;
  LatArgs<OutT> a;
  a.halves = H;
  a.n_units = n_units;
  a.m = h.m;
  a.src_xy = src;
  a.out = out;
  a.field_stride = (long long)nx * ny;
  a.err_flag = &err;
  const uint64_t epoch = 0x5A17000000000000ull + 7 + seed;
  a.unit_blocks = lat_unit_blocks(nx, ny);
  std::vector<vhp::lanes::Tagged> lines((size_t)a.unit_blocks * n_units * 64 + 64);
  for (size_t k = 0; k < lines.size(); ++k) { lines[k].v = std::numeric_limits<double>::quiet_NaN(); lines[k].tag = (k % 5 == 0) ? 0 : epoch - 1 - (k % 3); }
  a.lines = lines.data();
  a.epoch = epoch;
  a.src_index = nullptr;
  a.skip = nullptr;
  a.dead_cells_are_zero = false;
  a.strip_times = nullptr;
  a.dmap = h.diag.data();
  std::vector<std::vector<double>> lds(G, std::vector<double>(L.total, std::numeric_limits<double>::quiet_NaN()));
  const int WT = W * WorkerT::kRoles;  // wavefronts of a workgroup: the sweepers and, in the band sweep, a storer beside each
  std::vector<LatCo<WorkerT>> workers((size_t)G * WT);
  std::vector<Coro> coros((size_t)G * WT);
  for (int gI = 0; gI < G; ++gI) {
    WorkerT::clear(lds[gI].data(), L, 0, 1);
    for (int w = 0; w < WT; ++w) {
      LatCo<WorkerT>& wk = workers[(size_t)gI * WT + w];
      wk.wk.init(a, lds[gI].data(), L, w);
      wk.unit = gI;
      Coro& c = coros[(size_t)gI * WT + w];
      c.stack.reset(new char[kStack]);
      c.entry = lat_entry<WorkerT>;
      c.arg = &wk;
      getcontext(&c.ctx);
      c.ctx.uc_stack.ss_sp = c.stack.get();
      c.ctx.uc_stack.ss_size = kStack;
      c.ctx.uc_link = nullptr;
      makecontext(&c.ctx, trampoline, 0);
    }
  }
  vhp::lanes::sim_hooks().yield = hook_yield;
  vhp::lanes::sim_hooks().progress = hook_progress;
  vhp::lanes::sim_hooks().point = hook_point;
  vhp::lanes::store_stats() = vhp::lanes::StoreStats();
  vhp::lanes::sim_counts() = vhp::lanes::SimCounts();
  g_rng = seed * 2654435761u + 12345u;
  g_point_mode = (policy & 8) ? 1 : (policy & 16) ? 2 : 0;
  g_progress = g_switches = 0;
  const int n = G * WT, mode = policy & 7;
  int cur = mode == 1 ? n - 1 : 0, alive = n, burst = 0;
  long long last_progress = 0, stale = 0, deadlock = 0;
  while (alive > 0) {
    if (mode == 0) cur = (cur + 1) % n;
    else if (mode == 1) cur = (cur + n - 1) % n;
    else if (mode == 2) cur = (int)(lcg() % n);
    else if (mode == 3) { if (g_progress == last_progress) cur = (cur + 1) % n; }
    else { if (burst-- <= 0) { cur = (int)(lcg() % n); burst = (int)(lcg() % 6); } }
    int tries = 0;
    while (coros[cur].done && tries++ < n) cur = mode == 1 ? (cur + n - 1) % n : (cur + 1) % n;  // (wavefronts that have returned are skipped in the policy's direction)
    if (coros[cur].done) break;
    last_progress = g_progress;
    g_cur = &coros[cur];
    swapcontext(&g_sched, &g_cur->ctx);
    if (coros[cur].done) --alive;
    if (g_progress == last_progress) { if (++stale > 4000LL * n) { deadlock = 1; break; } } else stale = 0;
  }
  vhp::lanes::sim_hooks() = vhp::lanes::SimHooks();
  if (deadlock && getenv("VHP_SIM_DUMP")) {  // progress words of every workgroup, for debugging a stuck schedule
    for (int gI = 0; gI < G; ++gI) {
      Shared sh;
      sh.lds = lds[gI].data();
      sh.L = L;
      const int s_ = (gI / H) / kUnits, qo = (gI / H) % kUnits;
      UnitGeo ug;
      ug.init(nx, ny, qo, src[2 * s_], src[2 * s_ + 1]);
      fprintf(stderr, "unit %d (source %d,%d qo %d): strips %d diag ready %d\n   prog:", gI, src[2 * s_], src[2 * s_ + 1], qo, ug.n_strips, sh.ctx(0)[kDiagReady]);
      for (int p = 0; p < ug.n_strips && p < L.S; ++p) fprintf(stderr, " %d", sh.prog(0)[p]);
      fprintf(stderr, "\n   alive:");
      for (int w = 0; w < WT; ++w) fprintf(stderr, " %d", coros[(size_t)gI * WT + w].done ? 0 : 1);
      fprintf(stderr, "\n");
    }
  }
  if (stats) {
    stats[0] = g_switches;
    stats[1] = g_progress;
    stats[2] = deadlock;
    stats[3] = vhp::lanes::store_stats().n16;
    stats[4] = vhp::lanes::store_stats().n8;
    stats[5] = err;
    stats[6] = vhp::lanes::sim_counts().c[4];  // strips that died (stopped sweeping: all zeros from there on)
    for (int k = 0; k < 4; ++k) stats[7 + k] = vhp::lanes::sim_counts().c[k];
  }
  if (vhp::lanes::store_stats().misaligned) return 3;  // a pair stored off the grid of its own size
  return 0;
}

}  // namespace

// (the ODD build of the kernel where the launch needs it, as launch_lat_t picks it: vhp_lat.hip)
template <typename OutT>
int run_lat(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, OutT* out, int W, int policy, uint32_t seed, long long* stats, bool bands) {
  const bool odd = lat_needs_odd<OutT>(nx, (long long)nx * ny, out);
  if (bands)
    return g_lat_halves > 1 ? (odd ? run_lat_t<OutT, true, BandWorker<OutT, true, true>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats)
                                   : run_lat_t<OutT, false, BandWorker<OutT, false, true>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats))
                            : (odd ? run_lat_t<OutT, true, BandWorker<OutT, true, false>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats)
                                   : run_lat_t<OutT, false, BandWorker<OutT, false, false>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats));
  return odd ? run_lat_t<OutT, true, LatWorker<OutT, true>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats)
             : run_lat_t<OutT, false, LatWorker<OutT, false>>(occ, nx, ny, src, n_src, out, W, policy, seed, stats);
}

extern "C" {

// workgroups per unit of the band sweep's next runs (1 or 2: LatArgs::halves)
void vhp_sim_set_lat_halves(int h) { g_lat_halves = h; }

// The latency sweep: n_src * 8 workgroups of W wavefronts, one per unit.  Arguments and stats as vhp_sim_pool_sweep.
int vhp_sim_lat_sweep(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, int dtype, void* out, int W, int policy, unsigned seed,
                      long long* stats) {
  if (!occ || !src || !out || nx <= 0 || ny <= 0 || W < 2 || W > 16 || W * kXRows * kTStride < (nx < ny ? nx : ny)) return 1;
  if (dtype == 0) return run_lat<double>(occ, nx, ny, src, n_src, static_cast<double*>(out), W, policy, seed, stats, false);
  return run_lat<float>(occ, nx, ny, src, n_src, static_cast<float*>(out), W, policy, seed, stats, false);
}

// The latency sweep in bands (csrc/vhp_band.hpp): the same launch shape, arguments and stats.
int vhp_sim_band_sweep(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, int dtype, void* out, int W, int policy, unsigned seed,
                       long long* stats) {
  if (!occ || !src || !out || nx <= 0 || ny <= 0 || W < 1 || W > 16) return 1;
  if (dtype == 0) return run_lat<double>(occ, nx, ny, src, n_src, static_cast<double*>(out), W, policy, seed, stats, true);
  return run_lat<float>(occ, nx, ny, src, n_src, static_cast<float*>(out), W, policy, seed, stats, true);
}

// out: n_src fields of nx*ny elements (dtype 0 = double, 1 = float), pre-filled by the caller (NaN: an unwritten cell shows).
// W wavefronts per workgroup, C contexts, G workgroups sharing the queue.  stats (11 entries, may be null):
// coroutine switches, progress events, deadlock (0/1), 16-byte / 8-byte store instructions, the error flag, units pulled.
int vhp_sim_pool_sweep(const uint8_t* occ, int nx, int ny, const int32_t* src, int n_src, int dtype, void* out, int W, int C, int G,
                       int policy, unsigned seed, long long* stats) {
  if (!occ || !src || !out || nx <= 0 || ny <= 0 || W < 1 || W > 16 || C < 1 || C > 16 || G < 1) return 1;
  if (dtype == 0) return run_batch<double>(occ, nx, ny, src, n_src, static_cast<double*>(out), W, C, G, policy, seed, stats);
  return run_batch<float>(occ, nx, ny, src, n_src, static_cast<float*>(out), W, C, G, policy, seed, stats);
}

int vhp_sim_pool_lds_bytes(int nx, int ny, int W, int C) { return make_layout(W, C, nx, ny).total * 8; }

}  // extern "C"
