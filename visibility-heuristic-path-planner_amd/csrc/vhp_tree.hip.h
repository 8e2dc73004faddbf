// vhp_tree.hip.h -- path lengths to every cell and paths to any goal, from the tree a planner solve leaves in device memory
// (vhp_planner_length_fields, vhp_planner_goal_paths; the contract and the bodies are vhp_tree.hpp's).  The host route to the same
// numbers copies 8 * nx * ny bytes per query behind a widening pass and runs vhp_reconstruct_path once per cell on the host.
//   vhp_tree_tables : one workgroup per query.  parent[t] for every pivot (paths_parent_entry: the only gathers from the label field),
//                     then depth[t] by a walk bounded by n_pivots + 2 hops (tree_depth_entry), then cum[t] level by level behind
//                     barriers (tree_cum_entry: level l reads only level l - 1).  Rebuilt by every call: nothing is cached, so nothing
//                     has to be invalidated.
//   vhp_tree_fields : the streaming kernel.  Grid (tile of kTreeTile cells, query); a thread takes kTreeCellsPerThread groups of 4
//                     consecutive cells: one 16-byte label load, four table lookups + eval_d, two 16-byte length stores and one 16-byte
//                     count store per group.  The query's table (depth, cum, pivot coordinates: 20 bytes per pivot) is staged in LDS
//                     when it has at most kTreeLdsPivots entries, read through L2 otherwise.
//   vhp_tree_goals  : one thread per goal {q, x, y}: status, count and length from the table, the points written straight into place.
// All three are thin wrappers over vhp_tree.hpp, which the host compiler builds into the tests' driver.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vhp.h"
#include "vhp_paths.hip.h"
#include "vhp_tree.hpp"

namespace vhp {

static_assert(kTreeErrEndOob == VHP_ERR_END_OOB, "vhp_tree.hpp restates vhp.h's codes");

// LDS staging bound of vhp_tree_fields: tables of up to 1024 pivots, 20 bytes each = 20 KiB per workgroup.  By the arithmetic, eight
// workgroups of 256 threads -- the CU's full 32 wavefronts -- then hold 160 KiB, all of a CU's LDS and no more, so the static
// allocation should not lower the resident wavefronts.  NOT MEASURED: neither that residency, nor whether staging beats reading a
// table of a few KB through L2.  Most planner solves end after 3-250 pivots; a table of 1024 pivots or more (a long solve on a
// cluttered map, a fast speculative solve with a large max_iter) is read through L2.  Both branches are tested against the oracle at
// every cell: staged tables of up to 984 entries, tables of 1038 to 2834 entries through L2, and launches that mix the two under the
// stride max_nb + 1 (tests/test_gpu_long_solves.py).
constexpr uint32_t kTreeLdsPivots = 1024;
constexpr int kTreeThreads = 256;
constexpr int kTreeCellsPerThread = 16;                          // four groups of four consecutive cells
constexpr uint32_t kTreeTile = kTreeThreads * kTreeCellsPerThread;   // cells per workgroup, a multiple of 4: tiles keep a field's alignment

// One call's view: the solve (PathsDev: labels, pivots, every query's slot or validation code and n_pivots) and the tables of the
// queries q_first .. q_first + n_q - 1, query q's at entry (q - q_first) * (p.max_nb + 1).
struct TreeDev {
  PathsDev p;
  int q_first, n_q;
  uint32_t* parent;
  uint32_t* depth;
  double* cum;
};

struct TreeFieldArgs {
  TreeDev t;
  double* length;      // n_q fields of nx * ny, packed, in query order; either may be null
  uint32_t* n_path;
};

struct TreeGoalArgs {
  TreeDev t;           // (q_first = 0, n_q = all queries of the solve)
  const int32_t* goals;   // n_goals x {q, x, y}
  int n_goals;
  int32_t* path_xy;    // goal g's points at path_xy + 2 * g * cap; any output may be null
  uint32_t cap;
  uint32_t* n_path;
  double* length;
  int32_t* status;
};

__global__ void __launch_bounds__(kTreeThreads) vhp_tree_tables(TreeDev a) {
  __shared__ uint32_t deepest;
  const int q = a.q_first + (int)blockIdx.x;
  const int slot = a.p.slot[q];
  if (slot < 0) return;   // (the whole workgroup: no barrier is left waiting)
  const uint32_t nb = a.p.nb[q];
  const size_t at = (size_t)blockIdx.x * ((size_t)a.p.max_nb + 1);
  const uint32_t* label = a.p.label + (size_t)slot * a.p.label_stride;
  const int32_t* pivots = a.p.pivots + (size_t)slot * a.p.pivot_stride;
  uint32_t* parent = a.parent + at;
  uint32_t* depth = a.depth + at;
  double* cum = a.cum + at;
  if (threadIdx.x == 0) deepest = 0;
  for (uint32_t t = threadIdx.x; t <= nb; t += kTreeThreads) parent[t] = paths_parent_entry(label, pivots, t, a.p.nx, a.p.ny);
  __syncthreads();
  for (uint32_t t = threadIdx.x; t <= nb; t += kTreeThreads) {
    const uint32_t d = tree_depth_entry(parent, nb, t);
    depth[t] = d;
    cum[t] = 0.0;
    if (d != kTreeInvalid) atomicMax(&deepest, d);
  }
  __syncthreads();
  const uint32_t deep = deepest;   // (uniform: the loop's barriers are reached by every thread)
  for (uint32_t level = 1; level <= deep; ++level) {
    for (uint32_t t = threadIdx.x; t <= nb; t += kTreeThreads)
      if (depth[t] == level) cum[t] = tree_cum_entry(parent, pivots, cum, t);
    __syncthreads();
  }
}

// One tile of one query's field.  label null: a query without results, the filler everywhere.  vec: the query's label field and both
// output fields start on 16-byte boundaries (tiles start at multiples of 4 cells, so every full group of the tile is aligned then).
__device__ __forceinline__ void tree_fields_tile(const uint32_t* label, uint32_t nb, const uint32_t* depth, const double* cum, const int32_t* xy,
                                                 double* length, uint32_t* n_path, uint32_t tile_base, uint32_t cells, uint32_t nx, bool vec) {
#pragma unroll
  for (int j = 0; j < kTreeCellsPerThread / 4; ++j) {
    const uint32_t g = tile_base + 4u * ((uint32_t)j * kTreeThreads + threadIdx.x);
    if (g >= cells) break;
    uint32_t x = g % nx, y = g / nx;
    if (vec && g + 4 <= cells) {
      uint32_t lab[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
      if (label) {
        const uint4 v = *reinterpret_cast<const uint4*>(label + g);
        lab[0] = v.x; lab[1] = v.y; lab[2] = v.z; lab[3] = v.w;
      }
      uint32_t n[4];
      double len[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        tree_cell(lab[k], (int)x, (int)y, nb, depth, cum, xy, &n[k], &len[k]);
        if (++x == nx) { x = 0; ++y; }
      }
      if (length) {
        *reinterpret_cast<double2*>(length + g) = make_double2(len[0], len[1]);
        *reinterpret_cast<double2*>(length + g + 2) = make_double2(len[2], len[3]);
      }
      if (n_path) *reinterpret_cast<uint4*>(n_path + g) = make_uint4(n[0], n[1], n[2], n[3]);
    } else {
      for (uint32_t c = g; c < g + 4 && c < cells; ++c) {
        uint32_t n;
        double len;
        tree_cell(label ? label[c] : 0xffffffffu, (int)x, (int)y, nb, depth, cum, xy, &n, &len);
        if (length) length[c] = len;
        if (n_path) n_path[c] = n;
        if (++x == nx) { x = 0; ++y; }
      }
    }
  }
}

__global__ void __launch_bounds__(kTreeThreads) vhp_tree_fields(TreeFieldArgs a) {
  __shared__ double s_cum[kTreeLdsPivots];
  __shared__ int32_t s_xy[2 * kTreeLdsPivots];
  __shared__ uint32_t s_depth[kTreeLdsPivots];
  const int q = a.t.q_first + (int)blockIdx.y;
  const int slot = a.t.p.slot[q];
  const uint32_t cells = (uint32_t)a.t.p.nx * (uint32_t)a.t.p.ny;   // (sides up to VHP_MAX_SIDE = 8192: 2^26 cells at most)
  const size_t field = (size_t)blockIdx.y * cells;
  double* length = a.length ? a.length + field : nullptr;
  uint32_t* n_path = a.n_path ? a.n_path + field : nullptr;
  const uint32_t* label = slot >= 0 ? a.t.p.label + (size_t)slot * a.t.p.label_stride : nullptr;
  const bool vec = ((reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(length) | reinterpret_cast<uintptr_t>(n_path)) & 15) == 0;
  const uint32_t tile_base = blockIdx.x * kTreeTile;
  if (slot < 0) {
    tree_fields_tile(nullptr, 0, nullptr, nullptr, nullptr, length, n_path, tile_base, cells, (uint32_t)a.t.p.nx, vec);
    return;
  }
  const uint32_t nb = a.t.p.nb[q];
  const size_t at = (size_t)blockIdx.y * ((size_t)a.t.p.max_nb + 1);
  const int32_t* pivots = a.t.p.pivots + (size_t)slot * a.t.p.pivot_stride;
  if (nb < kTreeLdsPivots) {
    for (uint32_t t = threadIdx.x; t <= nb; t += kTreeThreads) {
      s_cum[t] = a.t.cum[at + t];
      s_depth[t] = a.t.depth[at + t];
      s_xy[2 * t] = pivots[2 * (size_t)t];
      s_xy[2 * t + 1] = pivots[2 * (size_t)t + 1];
    }
    __syncthreads();
    tree_fields_tile(label, nb, s_depth, s_cum, s_xy, length, n_path, tile_base, cells, (uint32_t)a.t.p.nx, vec);
  } else {
    tree_fields_tile(label, nb, a.t.depth + at, a.t.cum + at, pivots, length, n_path, tile_base, cells, (uint32_t)a.t.p.nx, vec);
  }
}

__global__ void __launch_bounds__(kTreeThreads) vhp_tree_goals(TreeGoalArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kTreeThreads + threadIdx.x;
  if (g >= (uint32_t)a.n_goals) return;
  const int q = a.goals[3 * (size_t)g], x = a.goals[3 * (size_t)g + 1], y = a.goals[3 * (size_t)g + 2];
  int st = VHP_ERR_ARG;
  uint32_t n = 0;
  double len = 0.0;
  if (q >= 0 && q < a.t.p.n_queries) {
    const int slot = a.t.p.slot[q];
    if (slot < 0) {
      st = -slot;   // a query without results: its validation code
    } else {
      const size_t at = (size_t)q * ((size_t)a.t.p.max_nb + 1);
      st = tree_goal_path(a.t.p.label + (size_t)slot * a.t.p.label_stride, a.t.parent + at, a.t.depth + at, a.t.cum + at,
                          a.t.p.pivots + (size_t)slot * a.t.p.pivot_stride, a.t.p.nb[q], a.t.p.nx, a.t.p.ny, x, y,
                          a.path_xy ? a.path_xy + 2 * (size_t)g * a.cap : nullptr, a.cap, &n, &len);
    }
  }
  if (a.status) a.status[g] = st;
  if (a.n_path) a.n_path[g] = n;
  if (a.length) a.length[g] = len;
}

// The context's scratch of the tree calls: the tables, and the host forms' staging (goals in, results out).  Grow-only, freed with the
// context.
// (a free waits for whatever still reads the memory)
struct TreeScratch {
  DevBuf<char> tab;
  DevBuf<char> io;
};

inline size_t tree_round16(size_t v) { return (v + 15) & ~(size_t)15; }

// Sizes the tables for queries q_first .. q_first + n_q - 1 of p and launches vhp_tree_tables; t comes back ready for the other two.
inline hipError_t tree_tables(TreeScratch& s, const PathsDev& p, int q_first, int n_q, hipStream_t stream, TreeDev* t) {
  t->p = p;
  t->q_first = q_first;
  t->n_q = n_q;
  t->p.max_nb = 0;
  bool any = false;
  for (int q = q_first; q < q_first + n_q; ++q)
    if (p.slot[q] >= 0) { t->p.max_nb = std::max(t->p.max_nb, p.nb[q]); any = true; }
  const size_t entries = (size_t)n_q * ((size_t)t->p.max_nb + 1);
  if (hipError_t e = s.tab.grow(entries * 16); e != hipSuccess) return e;
  t->cum = reinterpret_cast<double*>(s.tab.get());
  t->parent = reinterpret_cast<uint32_t*>(s.tab.get() + entries * 8);
  t->depth = t->parent + entries;
  if (!any) return hipSuccess;
  hipLaunchKernelGGL(vhp_tree_tables, dim3(n_q), dim3(kTreeThreads), 0, stream, *t);
  return hipGetLastError();
}

// vhp_planner_length_fields_device: tables, then the field kernel into the caller's buffers.
inline hipError_t tree_fields_launch(TreeScratch& s, const PathsDev& p, int q_first, int n_q, hipStream_t stream, double* length, uint32_t* n_path) {
  TreeFieldArgs a{};
  if (hipError_t e = tree_tables(s, p, q_first, n_q, stream, &a.t); e != hipSuccess) return e;
  a.length = length;
  a.n_path = n_path;
  const size_t cells = (size_t)p.nx * p.ny;
  hipLaunchKernelGGL(vhp_tree_fields, dim3((unsigned)((cells + kTreeTile - 1) / kTreeTile), n_q), dim3(kTreeThreads), 0, stream, a);
  return hipGetLastError();
}

// The host form: the same launches into staging, one copy per output straight into the caller's arrays, one synchronisation.
inline hipError_t tree_fields_host(TreeScratch& s, const PathsDev& p, int q_first, int n_q, hipStream_t stream, double* length, uint32_t* n_path) {
  const size_t n = (size_t)n_q * p.nx * p.ny;
  const size_t len_bytes = length ? tree_round16(8 * n) : 0, bytes = len_bytes + (n_path ? 4 * n : 0);
  if (hipError_t e = s.io.grow(bytes); e != hipSuccess) return e;
  double* d_len = length ? reinterpret_cast<double*>(s.io.get()) : nullptr;
  uint32_t* d_cnt = n_path ? reinterpret_cast<uint32_t*>(s.io.get() + len_bytes) : nullptr;
  if (hipError_t e = tree_fields_launch(s, p, q_first, n_q, stream, d_len, d_cnt); e != hipSuccess) return e;
  if (length)
    if (hipError_t e = hipMemcpyAsync(length, d_len, 8 * n, hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
  if (n_path)
    if (hipError_t e = hipMemcpyAsync(n_path, d_cnt, 4 * n, hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

// vhp_planner_goal_paths_device: tables of every query of the solve, then one thread per goal into the caller's buffers.
inline hipError_t tree_goals_launch(TreeScratch& s, const PathsDev& p, hipStream_t stream, TreeGoalArgs a) {
  if (hipError_t e = tree_tables(s, p, 0, p.n_queries, stream, &a.t); e != hipSuccess) return e;
  hipLaunchKernelGGL(vhp_tree_goals, dim3((unsigned)(((size_t)a.n_goals + kTreeThreads - 1) / kTreeThreads)), dim3(kTreeThreads), 0, stream, a);
  return hipGetLastError();
}

// The host form (every goal's q already checked against the solve): the goals go up behind the staging of the results (PathStaging,
// a row per goal), the launches run into it.
inline hipError_t tree_goals_host(TreeScratch& s, const PathsDev& p, hipStream_t stream, const int32_t* goals, int n_goals, int32_t* path_xy,
                                  uint32_t cap, uint32_t* n_path, double* length, int32_t* status) {
  const size_t G = (size_t)n_goals;
  const PathStaging st(p, G, path_xy, cap);
  const size_t out_bytes = tree_round16(st.bytes());
  if (hipError_t e = s.io.grow(out_bytes + 12 * G); e != hipSuccess) return e;
  int32_t* d_goals = reinterpret_cast<int32_t*>(s.io.get() + out_bytes);
  if (hipError_t e = hipMemcpyAsync(d_goals, goals, 12 * G, hipMemcpyHostToDevice, stream); e != hipSuccess) return e;
  TreeGoalArgs a{};
  a.goals = d_goals;
  a.n_goals = n_goals;
  st.attach(a, s.io.get());
  if (hipError_t e = tree_goals_launch(s, p, stream, a); e != hipSuccess) return e;
  return st.copy_out(s.io.get(), stream, path_xy, cap, n_path, length, status);
}

}  // namespace vhp
