// vhp_paths.hip.h -- the paths of planner solves, reconstructed where the results are: in device memory, all queries of a solve in
// one launch sequence (vhp_planner_path, vhp_planner_batch_paths, vhp_planner_maps_batch_paths).  The host route to a path copies
// 8 * nx * ny bytes per query behind a widening pass (vhp_planner_batch_results) and then reads at most n_pivots + 2 of those labels
// (vhp_reconstruct_path); this one moves 8 * cap + 16 bytes per query.
//   vhp_paths_parents : thread (k, q): entry k of query q's parent table (vhp_paths.hpp paths_parent_entry) -- every trip into a label
//                       field of nx * ny cells is made here, all of them at once;
//   vhp_paths_walk    : one wavefront per query, lane 0 walks (paths_walk: a chain of dependent loads through a table of a few KB) and
//                       adds the segments in path order; a query without results writes its validation code and zeros.
// Both are thin wrappers: the bodies are vhp_paths.hpp's, which the host compiler builds into the tests' driver.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "vhp.h"
#include "vhp_paths.hpp"
#include "vhp_planner_batch.hip.h"

namespace vhp {

static_assert(kPathsOk == VHP_OK && kPathsErrArg == VHP_ERR_ARG && kPathsErrTooLarge == VHP_ERR_TOO_LARGE, "vhp_paths.hpp restates vhp.h's codes");

// One call's view of a solve: the arrays hold one slot per query with results, label_stride / pivot_stride entries apart.
struct PathsDev {
  const uint32_t* label;
  const int32_t* pivots;
  size_t label_stride, pivot_stride;
  const BatchQuery* query;   // the end of slot k is query[k]'s; null: one query, its end is (end_x, end_y)
  int end_x, end_y;
  int nx, ny;
  int n_queries;
  uint32_t max_nb;           // the largest n_pivots of the call: the scratch of a query is sized by it
  uint32_t* scratch;         // per QUERY: max_nb + 1 parents, then 2 * (max_nb + 3) ints of the walk's points end-first
  // the caller's (or the host form's staging) buffers; any may be null
  int32_t* path_xy;
  uint32_t cap;
  uint32_t* n_path;
  double* length;
  int32_t* status;
  int16_t slot[kBatchMaxQueries];    // >= 0: the query's slot; < 0: minus the code its validation failed with (no results)
  uint32_t nb[kBatchMaxQueries];     // its n_pivots as the solve left it
};

__host__ __device__ inline size_t paths_scratch_words(uint32_t max_nb) { return (size_t)max_nb + 1 + 2 * ((size_t)max_nb + 3); }

__global__ void __launch_bounds__(256) vhp_paths_parents(PathsDev p) {
  const int q = (int)blockIdx.y;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  const int slot = p.slot[q];
  if (slot < 0 || k > p.nb[q]) return;
  p.scratch[(size_t)q * paths_scratch_words(p.max_nb) + k] =
      paths_parent_entry(p.label + (size_t)slot * p.label_stride, p.pivots + (size_t)slot * p.pivot_stride, k, p.nx, p.ny);
}

__global__ void __launch_bounds__(64) vhp_paths_walk(PathsDev p) {
  const int q = (int)blockIdx.x;
  if (threadIdx.x != 0) return;
  const int slot = p.slot[q];
  int st;
  uint32_t n = 0;
  double len = 0.0;
  if (slot < 0) {
    st = -slot;
  } else {
    const int ex = p.query ? p.query[slot].end_x : p.end_x, ey = p.query ? p.query[slot].end_y : p.end_y;
    uint32_t* parent = p.scratch + (size_t)q * paths_scratch_words(p.max_nb);
    const uint32_t end_label = p.label[(size_t)slot * p.label_stride + (size_t)ex + (size_t)ey * p.nx];
    st = paths_walk(end_label, parent, p.pivots + (size_t)slot * p.pivot_stride, p.nb[q], ex, ey,
                    reinterpret_cast<int32_t*>(parent + p.max_nb + 1), p.path_xy ? p.path_xy + 2 * (size_t)q * p.cap : nullptr, p.cap, &n, &len);
  }
  if (p.status) p.status[q] = st;
  if (p.n_path) p.n_path[q] = n;
  if (p.length) p.length[q] = len;
}

// The context's scratch of the path calls: the parent tables and walk buffers, and the host forms' staging.  Grow-only; sized by pivots
// and queries, not by the grid, so it outlives the maps (freed with the context).
struct PathsScratch {
  DevBuf<uint32_t> d;
  DevBuf<char> out;
};

// Launches the two kernels for p (slot, nb, the solve's arrays, the output pointers filled in by the caller) on stream.
inline hipError_t paths_launch(PathsScratch& s, PathsDev p, hipStream_t stream) {
  p.max_nb = 0;
  bool any = false;
  for (int q = 0; q < p.n_queries; ++q)
    if (p.slot[q] >= 0) { p.max_nb = std::max(p.max_nb, p.nb[q]); any = true; }
  const size_t bytes = (size_t)p.n_queries * paths_scratch_words(p.max_nb) * sizeof(uint32_t);
  if (hipError_t e = s.d.grow(bytes); e != hipSuccess) return e;   // (a free waits for whatever still reads the memory)
  p.scratch = s.d.get();
  if (any) {
    hipLaunchKernelGGL(vhp_paths_parents, dim3((p.max_nb + 1 + 255) / 256, p.n_queries), dim3(256), 0, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vhp_paths_walk, dim3(p.n_queries), dim3(64), 0, stream, p);
  return hipGetLastError();
}

// The staging of the host forms of the path and the goal calls (vhp_tree.hip.h), n rows of results -- a row per query or per goal -- in
// one piece of device memory: every row's length (8 bytes), status (4) and n_path (4), then scap points of 8 bytes per row.
struct PathStaging {
  size_t n;
  bool points;     // the caller takes the points (path_xy)
  uint32_t scap;
  size_t head() const { return 16 * n; }
  size_t bytes() const { return head() + 8 * (size_t)scap * n; }

  // For the paths of p's solve, `cap` points per row asked for (none without path_xy).
  // (no path has more than max_nb + 3 points: room beyond that would only be copied; a path of more than `cap` points still exceeds the
  // staging's room, as scap < cap only where no path reaches scap)
  PathStaging(const PathsDev& p, size_t rows, const int32_t* path_xy, uint32_t cap) : n(rows), points(path_xy != nullptr) {
    uint32_t max_nb = 0;
    for (int q = 0; q < p.n_queries; ++q)
      if (p.slot[q] >= 0) max_nb = std::max(max_nb, p.nb[q]);
    scap = points ? (uint32_t)std::min<uint64_t>(cap, (uint64_t)max_nb + 3) : 0;
  }

  // Points the outputs of a launch (PathsDev, TreeGoalArgs) into staging at d.
  template <typename Args>
  void attach(Args& a, char* d) const {
    a.length = reinterpret_cast<double*>(d);
    a.status = reinterpret_cast<int32_t*>(d + 8 * n);
    a.n_path = reinterpret_cast<uint32_t*>(d + 12 * n);
    a.path_xy = points ? reinterpret_cast<int32_t*>(d + head()) : nullptr;
    a.cap = scap;
  }

  // ONE copy of at most n * (8 * cap + 16) bytes back from d, one synchronisation; only the points of a row whose status is VHP_OK
  // reach the caller's path_xy (`cap` points apart).
  hipError_t copy_out(const char* d, hipStream_t stream, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* status) const {
    std::vector<char> h(bytes());
    if (hipError_t e = hipMemcpyAsync(h.data(), d, h.size(), hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e;
    const double* hl = reinterpret_cast<const double*>(h.data());
    const int32_t* hs = reinterpret_cast<const int32_t*>(h.data() + 8 * n);
    const uint32_t* hn = reinterpret_cast<const uint32_t*>(h.data() + 12 * n);
    const int32_t* hp = reinterpret_cast<const int32_t*>(h.data() + head());
    for (size_t r = 0; r < n; ++r) {
      if (length) length[r] = hl[r];
      if (status) status[r] = hs[r];
      if (n_path) n_path[r] = hn[r];
      if (path_xy && hs[r] == VHP_OK) std::copy(hp + 2 * r * scap, hp + 2 * r * scap + 2 * (size_t)hn[r], path_xy + 2 * r * (size_t)cap);
    }
    return hipSuccess;
  }
};

// The host form: the same launches into staging.
inline hipError_t paths_host(PathsScratch& s, PathsDev p, hipStream_t stream, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length,
                             int32_t* status) {
  const PathStaging st(p, (size_t)p.n_queries, path_xy, cap);
  if (hipError_t e = s.out.grow(st.bytes()); e != hipSuccess) return e;
  st.attach(p, s.out.get());
  if (hipError_t e = paths_launch(s, p, stream); e != hipSuccess) return e;
  return st.copy_out(s.out.get(), stream, path_xy, cap, n_path, length, status);
}

}  // namespace vhp
