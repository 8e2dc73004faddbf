/* vhp.h -- C ABI of the MI355X visibility-sweep / visibility-heuristic-planner library
 * (libvhp_hip.so).  This is the drop-in boundary: plain pointers and sizes, no C++
 * or torch types.
 *
 * The reference (IbrahimSquared/visibility-heuristic-path-planner) has no FFI or
 * plugin interface; its de-facto boundary is the public surface of
 * vbs::visibilityBasedSolver (include/solver/visibilityBasedSolver.h:23-71), whose
 * methods return void and leave results in members.  Each entry point below names
 * the reference code it replaces.
 *
 * Conventions
 *   - grids are row-major, x fastest: index = x + y*nx (include/environment/field.h:24-29)
 *   - occupancy is the reference's "occupancy complement": 1 = free, 0 = blocked
 *     (environment.cpp:200-207), one uint8 per cell
 *   - sources / pivots are int32 (x, y) pairs (parser.h:9 `point`)
 *   - every call returns a vhp_status; vhp_last_error() gives the message
 *   - a context is bound to one GPU and is not thread-safe (the reference object is
 *     stateful and single-threaded as well, visibilityBasedSolver.h:148-171)
 *   - there is NO CPU fallback: without a usable HIP device vhp_create fails.
 */
#ifndef VHP_H
#define VHP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vhp_ctx vhp_ctx;

typedef enum vhp_status {
  VHP_OK = 0,
  VHP_ERR_ARG = 1,            /* null pointer / bad size / bad enum */
  VHP_ERR_SOURCE_OOB = 2,     /* a sweep source lies outside the grid */
  VHP_ERR_NOTHING_LIT = 3,    /* planner: no cell reached the threshold (reference: top() of an empty heap) */
  VHP_ERR_START_OOB = 10,     /* "Start point is out of bounds."        solver.cpp:89-95  */
  VHP_ERR_END_OOB = 11,       /* "End point is out of bounds."          solver.cpp:96-102 */
  VHP_ERR_START_OCCUPIED = 12,/* "Start point is not valid (occupied)"  solver.cpp:103-109 */
  VHP_ERR_END_OCCUPIED = 13,  /* "End point is not valid (occupied)"    solver.cpp:110-116 */
  VHP_ERR_MAX_ITER = 20,      /* "Max iters hit. ..."                   solver.cpp:134-139 */
  VHP_ERR_HIP = 100,          /* a HIP runtime call failed */
  VHP_ERR_NO_MAP = 101,       /* vhp_set_map has not been called */
  VHP_ERR_TOO_LARGE = 102     /* grid side exceeds VHP_MAX_SIDE */
} vhp_status;

/* which sweep: computeVisibility (solver.cpp:570-696) or
 * computeVisibilityUsingQueue (solver.cpp:701-893) */
typedef enum vhp_variant { VHP_SWEEP_FULL = 0, VHP_SWEEP_QUEUE = 1 } vhp_variant;

/* element type of the STORED field; arithmetic is always IEEE binary64 */
/* VHP_U8: one byte per cell, 1 = visible; only the ray-cast entry points (vhp_raycast_[maps_]batch[_device]) accept it */
typedef enum vhp_dtype { VHP_F64 = 0, VHP_F32 = 1, VHP_U8 = 2 } vhp_dtype;

#define VHP_MAX_SIDE 8192
#define VHP_UNLABELLED 1000000000000000ULL /* (size_t)1e15, solver.cpp:46 */

/* Replaces the visibilityBasedSolver constructor + reset() (solver.cpp:13-60).
 * device_ordinal: HIP device index. */
int vhp_create(int device_ordinal, vhp_ctx** out);
int vhp_destroy(vhp_ctx* ctx);
const char* vhp_last_error(const vhp_ctx* ctx);

/* Launch everything on the caller's HIP stream (hipStream_t as void*; NULL = the
 * context's own stream).  Lets a host framework time and order the work itself. */
int vhp_set_stream(vhp_ctx* ctx, void* hip_stream);

/* Replaces environment::getVisibilityField() hand-over (environment.h:58-60,
 * solver.cpp:14-17): uploads the occupancy complement and builds the bit-packed
 * row-major and column-major copies the kernels read.  The map is immutable until
 * the next vhp_set_map. */
int vhp_set_map(vhp_ctx* ctx, const uint8_t* occ_rowmajor, int nx, int ny);
/* Same, the uint8 map already resident in device memory. */
int vhp_set_map_device(vhp_ctx* ctx, const uint8_t* d_occ_rowmajor, int nx, int ny);

/* Replaces computeVisibility() / computeVisibilityUsingQueue() for a batch of
 * independent sources (the reference handles one source per call through the
 * member ls_, solver.cpp:214-218).  out holds n_src fields of nx*ny elements of
 * `dtype`, field s at out + s*nx*ny.  Cells the reference never writes (row 0 /
 * column 0 unless the source lies on them; for the queue variant
 * blocked and unreached cells) are returned as 0, i.e. the result of running the
 * reference on a freshly reset() solver. */
int vhp_sweep_batch(vhp_ctx* ctx, const int32_t* src_xy, int n_src, int variant, int dtype, void* out_host);
/* Device-resident form: d_src_xy and d_out are device pointers; asynchronous on the
 * context stream.  Sources are validated on the device; query with vhp_sync().  d_out may start at any element of the caller's
 * buffer (aligned to the element type, else VHP_ERR_ARG); fields that start on a 128-byte line, on a width that is a multiple of 8,
 * are stored fastest. */
int vhp_sweep_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, int n_src, int variant, int dtype, void* d_out);
/* Waits for the stream and returns the status of device-side validation
 * (VHP_ERR_SOURCE_OOB if any source of an earlier *_device call was out of range). */
int vhp_sync(vhp_ctx* ctx);

/* A stack of maps: n_maps maps of one nx x ny, map k at occ + k*nx*ny (1 = free, row-major), packed like vhp_set_map's map.
 * Context state of its own: vhp_set_maps replaces the previous stack and leaves the single map of vhp_set_map, the planner's
 * state and the batch planner's as they are (and vhp_set_map leaves the stack); vhp_destroy frees it.  n_maps < 1, a null
 * pointer or a side < 1: VHP_ERR_ARG; a side above VHP_MAX_SIDE: VHP_ERR_TOO_LARGE; a failed allocation: VHP_ERR_HIP, with
 * no stack set.  "field_stride" is left as it is. */
int vhp_set_maps(vhp_ctx* ctx, const uint8_t* occ, int n_maps, int nx, int ny);
/* Same, the uint8 maps already resident in device memory. */
int vhp_set_maps_device(vhp_ctx* ctx, const uint8_t* d_occ, int n_maps, int nx, int ny);
/* The stack of maps as windows of the single map, cut on the device from that map's packed copies (one bit per cell read, nothing
 * crosses to the host): n_windows maps of w x h, map k the window whose cell (0, 0) is cell (origin_xy[2k], origin_xy[2k+1]) of the
 * map of vhp_set_map.  Window cell (i, j) is the map's cell (ox + i, oy + j) where that lies inside the grid and blocked (0) where
 * it does not.  Every int32 origin is valid: a window may hang over any edge or lie wholly outside the grid (all blocked), and
 * nothing is validated per window.  The stack is word for word the one vhp_set_maps builds from the same windows given as bytes, and
 * the state is vhp_set_maps's: the call synchronises, replaces the previous stack (with its diagonal maps and the maps-batch planner's
 * results) and leaves the single map, the planner's state, the batch planner's and "field_stride" alone.  The stack is a copy, not a
 * view: a later vhp_set_map leaves it as it is.  Everything that runs on a stack runs on windows unchanged, IN WINDOW COORDINATES --
 * sources, queries, paths and hit cells count from the window's cell (0, 0); adding the origin back is the caller's job.
 * The sweep on a window equals the sweep on the whole map, bit for bit, on every window cell that is inside the grid and neither in
 * the window's nor in the grid's first row or column (those the reference's loops never write on whatever grid they run):
 * visibility within range r is a window of side 2 (r + 1) + 1 around the source.
 * No single map: VHP_ERR_NO_MAP; a null pointer, n_windows < 1, w < 1 or h < 1: VHP_ERR_ARG; w or h above VHP_MAX_SIDE:
 * VHP_ERR_TOO_LARGE; a failed allocation: VHP_ERR_HIP; on failure no stack is set.  Not timed: vhp_last_elapsed_ms keeps what it
 * had. */
int vhp_set_maps_windows(vhp_ctx* ctx, const int32_t* origin_xy, int n_windows, int w, int h);
/* Same, the origins already resident in device memory; returns when the stack is on the device, as vhp_set_maps_device does. */
int vhp_set_maps_windows_device(vhp_ctx* ctx, const int32_t* d_origin_xy, int n_windows, int w, int h);
/* Maps first .. first + n - 1 of the current stack, however it was made, unpacked to one byte per cell (1 = free, 0 = blocked) in
 * the layout vhp_set_maps takes: map first + k at occ_out + k*nx*ny of the stack's nx x ny.  Read from the row-packed copy; changes
 * no state.  No stack: VHP_ERR_NO_MAP; a range outside 0 .. n_maps-1, n < 1 or a null pointer: VHP_ERR_ARG. */
int vhp_maps_occupancy(vhp_ctx* ctx, int first, int n, uint8_t* occ_out);
/* Device-resident form: asynchronous on the context stream. */
int vhp_maps_occupancy_device(vhp_ctx* ctx, int first, int n, uint8_t* d_occ_out);

/* Obstacles grown by a robot's footprint, on the device (the configuration-space map: everything here plans for a point).  A
 * footprint is a set of integer offsets (dx, dy) picked by `shape` and one integer p >= 0:
 *   VHP_FOOT_DISC     dx*dx + dy*dy <= p        (p is the SQUARED radius in cells: every digital disc is reachable, no square root)
 *   VHP_FOOT_SQUARE   max(|dx|, |dy|) <= p
 *   VHP_FOOT_DIAMOND  |dx| + |dy| <= p
 * Its reach, the largest |dx| -- isqrt(p), p, p --, is at most VHP_MAX_INFLATE cells.  Cell (x, y) of the inflated map is blocked
 * exactly when some cell (x + dx, y + dy), (dx, dy) in the footprint, is blocked in the input.  Cells outside the grid count as FREE
 * (a map's edge is no wall) unless flags has VHP_INFLATE_BORDER, which makes them blocked: every cell within the footprint of the
 * edge is then blocked too.  p = 0 is the identity footprint: the same map, and the same changes of state.
 *
 * vhp_inflate_map replaces the single map by its inflation, computed from the row-packed copy.  Afterwards the context is in the
 * state vhp_set_map_device of the inflated bytes would leave: the uint8 map, both packed copies, the diagonal maps where the latency
 * sweep takes the grid, no host copy of the map, "field_stride" reset to 0, the results of the plain, speculative and batch solves
 * dropped; the stack of maps and its solves untouched.  Every later call on the single map is bit for bit what it is after
 * vhp_set_map of the inflated map.  Synchronous, as vhp_set_map is; not timed: vhp_last_elapsed_ms keeps what it had.
 * No map: VHP_ERR_NO_MAP; an unknown shape, p < 0, a reach above VHP_MAX_INFLATE or a flag bit other than VHP_INFLATE_BORDER:
 * VHP_ERR_ARG; a refused call changes nothing.  A failed HIP call: VHP_ERR_HIP, with the map as it was if the inflation itself
 * failed and no map set if the rebuild after it did (as a failed vhp_set_map leaves none).
 *
 * vhp_inflate_maps does the same to maps first .. first + n - 1 of the stack, whether it came from bytes or from windows; the
 * other maps stay word for word.  Both packed copies of the range are inflated into scratch and copied back, and the stack is then in
 * the state vhp_set_maps_device of the resulting bytes would leave: its lazily built diagonal maps and the maps batch's results are
 * gone, the single map, its solves and "field_stride" stay.  Synchronous, not timed.  No stack (a single map is none):
 * VHP_ERR_NO_MAP; a range outside 0 .. n_maps-1 or n < 1 (as vhp_maps_occupancy) or a bad footprint or flag (as above): VHP_ERR_ARG,
 * nothing changed.  A failed HIP call: VHP_ERR_HIP and the stack is EMPTY (no stack set), never a mix of old and new maps.
 *
 * How the calls compose.  Inflate the single map BEFORE cutting windows from it (vhp_set_maps_windows): a window of the inflated map
 * also holds the growth of obstacles that lie just outside the window, which inflating a cut window cannot know -- it sees the
 * window's cells outside the grid as the blocked cells the cut made them, and nothing beyond the window.  A fleet of K robot sizes on
 * one map: vhp_set_maps_windows with K origins (0, 0) and w, h = nx, ny (K device copies of the map), vhp_inflate_maps(k, 1, ...) per
 * size, then vhp_planner_solve_maps_batch with map_idx[q] = the class of query q's robot. */
typedef enum vhp_footprint { VHP_FOOT_DISC = 0, VHP_FOOT_SQUARE = 1, VHP_FOOT_DIAMOND = 2 } vhp_footprint;
#define VHP_MAX_INFLATE 64
#define VHP_INFLATE_BORDER 1
int vhp_inflate_map(vhp_ctx* ctx, int shape, int p, int flags);
int vhp_inflate_maps(vhp_ctx* ctx, int first, int n, int shape, int p, int flags);
/* The single map unpacked to one byte per cell (1 = free, 0 = blocked: normalised, whatever non-zero bytes vhp_set_map was given),
 * nx*ny bytes in the layout vhp_set_map takes.  Read from the row-packed copy; changes no state.  What shows an inflated map.
 * No map: VHP_ERR_NO_MAP; a null pointer: VHP_ERR_ARG. */
int vhp_map_occupancy(vhp_ctx* ctx, uint8_t* occ_out);
/* Device-resident form: asynchronous on the context stream. */
int vhp_map_occupancy_device(vhp_ctx* ctx, uint8_t* d_occ_out);

/* The clearance field: for every cell the distance to the nearest obstacle, in the terms of the footprints above -- the smallest p at
 * which vhp_inflate_map(shape, p, flags) would block the cell.  With the metric m(dx, dy) of `shape`,
 *   VHP_FOOT_DISC     dx*dx + dy*dy             (the SQUARED distance in cells)
 *   VHP_FOOT_SQUARE   max(|dx|, |dy|)
 *   VHP_FOOT_DIAMOND  |dx| + |dy|
 * c(x, y) is the minimum of m(dx, dy) over all (dx, dy) for which cell (x + dx, y + dy) is blocked; with VHP_INFLATE_BORDER in `flags`
 * every cell outside the grid counts as blocked, without it cells outside are free and contribute nothing.  The output holds c where
 * c <= p_max and VHP_CLEARANCE_FAR elsewhere: a blocked cell holds 0, an all-free map without the border flag is VHP_CLEARANCE_FAR
 * everywhere.  p_max has exactly the domain of vhp_inflate_map's p (a disc 0 .. 4224, a square or a diamond 0 .. 64: a reach of at most
 * VHP_MAX_INFLATE).  For every p <= p_max, (c > p) is, bit for bit, the map vhp_inflate_map(shape, p, flags) leaves: a robot of squared
 * radius p fits at a cell exactly when c > p there.  One field therefore answers collision checks for any radius, gives the largest
 * robot class that fits at a cell, and yields the K configuration-space maps of a fleet from one pass (compare against K values of p on
 * the device, then vhp_set_maps_device of the K masks).
 *
 * uint16_t per cell, nx*ny of them in the layout of vhp_map_occupancy; vhp_maps_clearance writes map first + k of the stack at
 * out + k*nx*ny (the stack's nx, ny), n maps, and nothing else.  Read from the row-packed copy; the calls change no state.  The host
 * forms are synchronous and not timed (vhp_last_elapsed_ms keeps what it had); the _device forms are asynchronous on the context's
 * stream, one kernel launch whatever n.  A null pointer, a d_out not aligned to 2 bytes, a range outside the stack or n < 1 (as
 * vhp_maps_occupancy), an unknown shape, p_max < 0, a reach above VHP_MAX_INFLATE or an unknown flag (as vhp_inflate_map): VHP_ERR_ARG;
 * no map (vhp_map_clearance) or no stack (vhp_maps_clearance): VHP_ERR_NO_MAP.  A refused call writes nothing. */
#define VHP_CLEARANCE_FAR 0xFFFF
int vhp_map_clearance(vhp_ctx* ctx, int shape, int p_max, int flags, uint16_t* out);
int vhp_map_clearance_device(vhp_ctx* ctx, int shape, int p_max, int flags, uint16_t* d_out);
int vhp_maps_clearance(vhp_ctx* ctx, int first, int n, int shape, int p_max, int flags, uint16_t* out);
int vhp_maps_clearance_device(vhp_ctx* ctx, int first, int n, int shape, int p_max, int flags, uint16_t* d_out);
/* Replaces computeVisibility() (solver.cpp:570-696) run on a different environment per source: field i is the sweep from
 * src_xy[2i..2i+1] on map map_idx[i] of the stack, bit for bit what vhp_set_map(that map) + vhp_sweep_batch(VHP_SWEEP_FULL,
 * dtype) gives.  Output layout, zero cells and n_src as in vhp_sweep_batch.  Always the front sweep (vhp_last_sweep_kernel
 * reports 1); the shape options apply as in vhp_sweep_batch, "kernel" is ignored.  A source outside the grid or a map index
 * outside 0..n_maps-1 leaves its field 0, the others are swept, and the call returns VHP_ERR_SOURCE_OOB.  No stack set:
 * VHP_ERR_NO_MAP. */
int vhp_sweep_maps_batch(vhp_ctx* ctx, const int32_t* src_xy, const int32_t* map_idx, int n_src, int dtype, void* out_host);
/* Device-resident form, as vhp_sweep_batch_device ("field_stride" and the alignment rule checked against the stack's nx*ny):
 * a rejected source's field is not written, and vhp_sync() reports VHP_ERR_SOURCE_OOB. */
int vhp_sweep_maps_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out);

/* Replaces solve() (solver.cpp:76-160) incl. updateVisibility() (:379-565), the
 * heap / top() arg-min (visibilityBasedSolver.h:16-21,138) and resetQueue().
 * Coordinates are FIELD coordinates (the mode-2 y flip of solver.cpp:83-86 is the
 * caller's).  Outputs (any may be NULL): came_from nx*ny (cameFrom_, VHP_UNLABELLED
 * where unlabelled), vis_global / vis_local nx*ny (visibility_global_, visibility_ of
 * the last pivot), pivots_xy 2*(max_iter+2) (lightSources_[0..*n_pivots], the last
 * entry is `end`, solver.cpp:141), *n_pivots = nb_of_sources_.
 * Returns VHP_OK, one of the four validation codes, VHP_ERR_MAX_ITER (outputs are
 * still filled) or VHP_ERR_NOTHING_LIT. */
int vhp_planner_solve(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold,
                      uint64_t max_iter, uint64_t* came_from, double* vis_global, double* vis_local,
                      int32_t* pivots_xy, uint32_t* n_pivots);

/* The same solve with every result left in device memory (a batched or multi-GPU planner consumes labels and union on
 * the GPU; the host copy of vhp_planner_solve costs 10x the device loop at 1000^2).  *n_pivots = nb_of_sources_.
 * vhp_planner_results_device then hands out the device arrays of the most recent solve on this context, valid until the
 * next solve or vhp_set_map: labels nx*ny uint32 (0xFFFFFFFF where the reference holds (size_t)1e15), vis_global and
 * vis_local nx*ny doubles, pivots_xy int32 pairs 0 .. n_pivots.  Any output pointer may be NULL. */
int vhp_planner_solve_device(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, uint64_t max_iter,
                             uint32_t* n_pivots);
int vhp_planner_results_device(vhp_ctx* ctx, const uint32_t** labels, const double** vis_global, const double** vis_local,
                               const int32_t** pivots_xy);

/* The speculative planner (the loop of solver.cpp:127-140 with every sweep launch taking the k - 1 best other candidates of
 * the last heuristic evaluation along; a launch sweeps k sources in the time it sweeps one).  k = 1, 2, 4 or 8.
 *   mode 0, exact: the extra fields go into a cache keyed by their source cell, and an iteration whose pivot is cached
 *     skips its sweep.  Every output equals vhp_planner_solve's bit for bit; only the number of sweep launches differs.
 *   mode 1, fast, NOT the reference's result: all k candidates of a launch are committed as pivots in that iteration, in
 *     rank order.  The outputs are a valid planner result (labels index pivots, every pivot was lit by an earlier one, the
 *     path reconstructs) but not the reference's pivots or path.
 * stats (may be NULL): [0] iterations whose pivot was cached, [1] iterations that swept, [2] fields swept.
 * pivots_xy: at least 2*(max_iter+2+8) ints -- in mode 1 an iteration commits up to k pivots before the max_iter test, so
 * *n_pivots can reach max_iter + 8.  Their launches take the latency sweep (8 k workgroups) wherever a batch of k would.  Measured
 * on maze_6 (threshold 0.1, 64 pivots; vhp_planner_solve 1.70 ms): mode 1 with k = 4 1.44 ms -- 149 pivots in 38 launches --, k = 2
 * 1.62; mode 0 2.44 ms: it sweeps k fields where the plain loop sweeps one and skips 13 of 64 sweeps, which does not pay there.  It
 * pays where pivots repeat (the reference's live-lock, threshold 0.25 on the same map: 3.8 ms against 5.6 until max_iter = 250; mode
 * 1 SOLVES that instance, 157 pivots in 1.51 ms).  DESIGN.md section 7.
 * Results stay on the device as with vhp_planner_solve_device (vhp_planner_results_device); host outputs may be NULL. */
int vhp_planner_solve_speculative(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, uint64_t max_iter,
                                  int k, int mode, uint64_t* came_from, double* vis_global, double* vis_local, int32_t* pivots_xy,
                                  uint32_t* n_pivots, int32_t* stats);

/* Many planner queries on one map in one call: Q independent solve()s, each giving exactly what vhp_planner_solve gives for it
 * alone (status, pivots, labels, union, last local field -- bit for bit).  queries: Q x {start_x, start_y, end_x, end_y} (field
 * coordinates); thresholds: Q doubles; max_iter shared.  status[q]: what vhp_planner_solve would return for query q alone (the four
 * validation codes, checked in the reference's order; VHP_OK, VHP_ERR_MAX_ITER, VHP_ERR_NOTHING_LIT); n_pivots[q]: its
 * nb_of_sources_ (0 for a query that failed validation).  These per-query outcomes go only into status[]: the call then returns
 * VHP_OK (vhp_last_error names the first query that failed validation).  The call itself fails with VHP_ERR_ARG (n_queries outside
 * 1..64, a null queries / thresholds / status / n_pivots, max_iter > 2^24), VHP_ERR_NO_MAP or VHP_ERR_HIP.
 * One iteration serves every query still running: ONE latency-sweep launch whose source g is query g's current pivot, then ONE
 * epilogue launch over all their states; the host polls every 8 iterations.  The queries run in groups of G, one group after the
 * other: G is the largest of 32, 16, 8, 4, 2 for which a sweep of G sources takes the latency sweep (vhp_last_sweep_kernel's rule)
 * and G queries' state -- 28 bytes per cell and the pivot list per query -- fits in a quarter of the free device memory, else 1;
 * vhp_set_option "planner_batch_group" (0 automatic, 1..32) caps it.  Where not even one source takes the latency sweep, every query
 * runs on the front sweep alone.  No result depends on G.  The results of ALL the batch's queries stay in device memory (28 bytes per
 * cell per query) until the next batch solve or vhp_set_map; the batch's state is its own: vhp_planner_results_device still returns
 * the last plain solve's.  vhp_last_elapsed_ms times the whole call; vhp_last_sweep_kernel says what swept its iterations (4 or 1).
 * vhp_planner_batch_results_device hands out query q's device arrays (the layout of vhp_planner_results_device), and
 * vhp_planner_batch_results copies them to the host in the layout of vhp_planner_solve's outputs (pivots_xy: n_pivots[q] + 1
 * pairs); any output pointer may be NULL.  Both return VHP_ERR_ARG for q outside 0..Q-1, for a query that failed validation, and
 * before any batch has been solved since the last vhp_set_map.
 * vhp_planner_batch_group (beyond the three calls the batch was specified with): the G the last batch solve ran with, 0 before any. */
int vhp_planner_solve_batch(vhp_ctx* ctx, const int32_t* queries, const double* thresholds, int n_queries, uint64_t max_iter,
                            int32_t* status, uint32_t* n_pivots);
int vhp_planner_batch_results_device(vhp_ctx* ctx, int q, const uint32_t** labels, const double** vis_global,
                                     const double** vis_local, const int32_t** pivots_xy);
int vhp_planner_batch_results(vhp_ctx* ctx, int q, uint64_t* came_from, double* vis_global, double* vis_local,
                              int32_t* pivots_xy);
int vhp_planner_batch_group(const vhp_ctx* ctx);

/* Many planner queries across a stack of maps in one call: query q runs on map map_idx[q] of the stack of vhp_set_maps and gives
 * exactly what vhp_set_map(that map) + vhp_planner_solve gives for it alone (status, pivots, labels, union, last local field -- bit
 * for bit).  Semantics as vhp_planner_solve_batch's, with these differences.  The four validation codes of status[q] are checked
 * against the query's own map.  The call fails with VHP_ERR_ARG also for a null map_idx and for any map_idx[q] outside
 * 0..n_maps-1 (checked on the host before anything runs), and with VHP_ERR_NO_MAP when no stack is set.  G follows
 * vhp_planner_solve_batch's rule on the stack's nx x ny, with the context's options ("planner_batch_group" caps it; "kernel" = 1
 * runs every query on the front sweep, G = 1); the sweep launch reads each query's map index on the device (vhp_lat_maps_sweep).
 * The first such call after a vhp_set_maps that takes the latency sweep builds the stack's diagonal maps (the latency sweep's copy
 * of every map, DiagMaps::words(nx, ny) words a map), kept until the next vhp_set_maps or vhp_destroy.  The results have state of
 * their own: they stay until the next maps-batch solve or vhp_set_maps; vhp_set_map leaves them alone, and this call leaves the
 * single map, the plain planner's results and vhp_planner_solve_batch's results and group alone.  vhp_last_elapsed_ms times the
 * whole call; vhp_last_sweep_kernel reports 4 or 1.  vhp_planner_maps_batch_results_device / vhp_planner_maps_batch_results /
 * vhp_planner_maps_batch_group are vhp_planner_batch_results_device / vhp_planner_batch_results / vhp_planner_batch_group for
 * the last maps batch (VHP_ERR_ARG before any since the last vhp_set_maps). */
int vhp_planner_solve_maps_batch(vhp_ctx* ctx, const int32_t* queries, const int32_t* map_idx, const double* thresholds,
                                 int n_queries, uint64_t max_iter, int32_t* status, uint32_t* n_pivots);
int vhp_planner_maps_batch_results_device(vhp_ctx* ctx, int q, const uint32_t** labels, const double** vis_global,
                                          const double** vis_local, const int32_t** pivots_xy);
int vhp_planner_maps_batch_results(vhp_ctx* ctx, int q, uint64_t* came_from, double* vis_global, double* vis_local,
                                   int32_t* pivots_xy);
int vhp_planner_maps_batch_group(const vhp_ctx* ctx);

/* Replaces reconstructPath() (solver.cpp:1183-1213): walks came_from -> pivots from
 * `end` until the label repeats; writes the path start-first into path_xy (capacity
 * cap points), its point count into *n_path, the summed eval_d length into *length.
 * pivots_xy holds entries 0 .. n_pivots (vhp_planner_solve's *n_pivots).  A label above
 * n_pivots (an unlabelled cell included) or a walk longer than n_pivots + 2 hops is
 * VHP_ERR_ARG; a path longer than cap is VHP_ERR_TOO_LARGE with *n_path = the size
 * needed and nothing written. */
int vhp_reconstruct_path(const uint64_t* came_from, const int32_t* pivots_xy, uint32_t n_pivots, int nx, int ny,
                         int end_x, int end_y, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length);

/* reconstructPath() (solver.cpp:1183-1213) on the device, for every query of a solve at once: the labels and pivots the solves leave
 * in device memory are walked there, and only the paths cross to the host (8 * cap + 16 bytes per query; the route through
 * vhp_planner_[maps_]batch_results + vhp_reconstruct_path copies 8 * nx * ny bytes per query behind a widening pass).
 *   vhp_planner_batch_paths        all Q queries of the last vhp_planner_solve_batch, in the batch's order
 *   vhp_planner_maps_batch_paths   the same for the last vhp_planner_solve_maps_batch
 *   vhp_planner_path               the last vhp_planner_solve / _solve_device / _solve_speculative of the context (Q = 1)
 * For query q the outputs are exactly what vhp_reconstruct_path(came_from_q, pivots_q, n_pivots[q], nx, ny, end_q, path, cap, &n, &len)
 * gives on the arrays the solve's host outputs / results call would copy out (the caller passes no coordinates: each query's end,
 * n_pivots -- the solve's own count, up to max_iter + 8 after the speculative solve's fast mode -- and arrays are the context's):
 *   path_status[q]: that call's return value.  VHP_OK; VHP_ERR_ARG for an unlabelled end (usual after VHP_ERR_MAX_ITER or
 *     VHP_ERR_NOTHING_LIT), a label above n_pivots (device labels are uint32 with 0xFFFFFFFF for (size_t)1e15: both are above), a pivot
 *     outside the grid or a walk of more than n_pivots + 2 hops -- the host's checks in the host's order, so no table, consistent or
 *     not, is read out of bounds; VHP_ERR_TOO_LARGE for a path of more than cap points.  A query that failed validation (no results):
 *     its validation code, with n_path[q] = 0 and length[q] = 0.
 *   path_xy + 2*q*cap: the points start-first, n_path[q] of them (cap points of room per query); written only where path_status[q]
 *     is VHP_OK.  The walk stops where the label repeats, as the host's, not "at the start".
 *   n_path[q], length[q]: the point count and the length -- eval_d per segment, added one after the other from the start's end of the
 *     path, so bit-identical to the host's sum.  On VHP_ERR_TOO_LARGE n_path[q] is the size needed and length[q] still the length; on
 *     VHP_ERR_ARG both are 0 (vhp_reconstruct_path leaves its outputs alone there).
 * path_xy may be NULL: counts and lengths only, cap ignored, no query reports VHP_ERR_TOO_LARGE.  n_path, length and path_status may
 * each be NULL.  The call returns VHP_OK when it ran -- per-query outcomes go only into path_status --, VHP_ERR_ARG for a null context
 * and before any such solve since the last vhp_set_map (vhp_set_maps for the maps batch), VHP_ERR_HIP on a runtime failure.
 * The host forms copy Q * (8 * min(cap, largest n_pivots + 3) + 16) bytes in one copy and synchronise once.  The _device forms take
 * device pointers, are asynchronous on the context's stream and write nothing but the caller's buffers.  Two small launches: a parent
 * table (the label of every pivot's cell, one thread each) and the walks (one wavefront per query); their scratch, 12 bytes per pivot
 * and query, belongs to the context.  No call changes any state of a solve: results, groups and vhp_last_sweep_kernel stay as they
 * were.  Not timed: vhp_last_elapsed_ms still reports the sweep or solve before it.  The mode-2 y flip stays the caller's.
 * (vhp_planner_solve_variant keeps host outputs and a stop rule of its own: not covered.) */
int vhp_planner_batch_paths(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status);
int vhp_planner_batch_paths_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length,
                                   int32_t* d_path_status);
int vhp_planner_maps_batch_paths(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status);
int vhp_planner_maps_batch_paths_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length,
                                        int32_t* d_path_status);
int vhp_planner_path(vhp_ctx* ctx, int32_t* path_xy, uint32_t cap, uint32_t* n_path, double* length, int32_t* path_status);
int vhp_planner_path_device(vhp_ctx* ctx, int32_t* d_path_xy, uint32_t cap, uint32_t* d_n_path, double* d_length, int32_t* d_path_status);

/* The whole tree of a solve, read from any cell: path lengths to every cell (a cost-to-come field per query) and paths to any goal.
 * A solve leaves a tree in device memory, not one path: every cell some pivot lit carries that pivot's label, every pivot's own cell the
 * label of the pivot that lit it.  The path calls above walk it from each query's `end` only; these walk it from any cell -- one start,
 * many goals -- and replace the reference's interface.m:141-162 (back-tracking cameFrom + pivots from a point the user chooses).
 * `solve` selects whose tree (vhp_solve_kind): VHP_SOLVE_PLAIN the last vhp_planner_solve / _solve_device / _solve_speculative of the
 * context (Q = 1), VHP_SOLVE_BATCH the last vhp_planner_solve_batch, VHP_SOLVE_MAPS_BATCH the last vhp_planner_solve_maps_batch;
 * lifetimes are those of the path calls (until the next such solve or vhp_set_map; vhp_set_maps for the maps batch).
 * For query q and cell (x, y) everything reported is exactly what
 *   vhp_reconstruct_path(came_from_q, pivots_q, n_pivots[q], nx, ny, x, y, path, cap, &n, &len)
 * gives on the arrays the solve's host outputs / results call would copy out: return value, point count, points, and the fp64 bits of
 * the length (eval_d per segment, added one after the other from the start's end of the path).  That call returns VHP_ERR_ARG for an
 * unlabelled cell (blocked cells and cells no pivot lit; usual far from the path, and everywhere unlit after VHP_ERR_MAX_ITER), a label
 * above n_pivots, a pivot outside the grid anywhere on the chain, and labels that form a cycle -- the host's checks, so no table,
 * consistent or not, is read out of bounds or walked without bound.
 *   vhp_planner_length_fields: queries q_first .. q_first + n_q - 1; each gets nx * ny doubles in `length` and nx * ny uint32 in `n_path`,
 *     packed, row-major, in query order (query q's field at (q - q_first) * nx * ny).  Either output may be NULL.  A cell whose call
 *     would return VHP_OK gets its length and point count (2 + the depth of its label in the tree); every other cell gets length = -1.0
 *     and n_path = 0; a query that failed validation (no results) gets that filler everywhere.  Returns VHP_OK when it ran;
 *     VHP_ERR_ARG for a null context, a selector that is no vhp_solve_kind, a range outside 0..Q-1 (n_q < 1 included), both outputs
 *     NULL, and before any such solve; VHP_ERR_HIP on a runtime failure.
 *   vhp_planner_goal_paths: goal g is the triple goals_qxy[3g .. 3g+2] = {q, x, y}; outputs per goal as vhp_planner_batch_paths' per query.
 *     path_status[g]: VHP_OK, VHP_ERR_ARG or VHP_ERR_TOO_LARGE as that call returns them; VHP_ERR_END_OOB for a goal outside the grid
 *     (the host call returns it before it walks); for a query without results its validation code, whatever the goal.  path_xy +
 *     2*g*cap: the points start-first, written only where path_status[g] is VHP_OK.  On VHP_ERR_TOO_LARGE n_path[g] is the size needed
 *     and length[g] still the length; on every other status but VHP_OK both are 0.  path_xy may be NULL: counts and lengths only, cap
 *     ignored, no goal reports VHP_ERR_TOO_LARGE.  n_path, length and path_status may each be NULL.  A q outside 0..Q-1: the host form
 *     checks every goal first and fails the call with VHP_ERR_ARG, nothing written; the _device form gives that goal the status
 *     VHP_ERR_ARG.  n_goals = 0 is VHP_OK with nothing written; n_goals < 0 or null goals: VHP_ERR_ARG.  Otherwise the call returns as
 *     vhp_planner_length_fields does -- per-goal outcomes go only into path_status.
 * The _device forms take device pointers (aligned to their element types, else VHP_ERR_ARG), are asynchronous on the context's stream
 * and write nothing but the caller's buffers -- asynchronous once the context's scratch has reached its size: the first call, and any
 * call with more pivots or queries than every call before it, frees and allocates the scratch, which waits for the device (as for the
 * path calls).  The host forms stage the results in device memory and synchronise once: length_fields makes one copy per output asked
 * for, straight into the caller's arrays (8 and 4 bytes per cell); goal_paths makes ONE copy of n_goals * (8 * min(cap, largest
 * n_pivots + 3) + 16) bytes.  Per call: one small launch that builds a
 * table of every pivot's depth, validity and running length from the root (20 bytes per pivot with its coordinates, plus its parent;
 * rebuilt every call, never cached; scratch of the context), then one streaming launch over the cells -- one label load, one table
 * lookup, one eval_d, one store per cell; fields that start on a 16-byte boundary are read and written 16 bytes at a time -- or one
 * thread per goal.  No call changes any state of a solve: results, groups and vhp_last_sweep_kernel stay as they were.  Not timed:
 * vhp_last_elapsed_ms still reports the sweep or solve before it.  The mode-2 y flip stays the caller's.
 * (vhp_planner_solve_variant keeps host outputs and a stop rule of its own: not covered.) */
typedef enum vhp_solve_kind { VHP_SOLVE_PLAIN = 0, VHP_SOLVE_BATCH = 1, VHP_SOLVE_MAPS_BATCH = 2 } vhp_solve_kind;
int vhp_planner_length_fields(vhp_ctx* ctx, int solve, int q_first, int n_q, double* length, uint32_t* n_path);
int vhp_planner_length_fields_device(vhp_ctx* ctx, int solve, int q_first, int n_q, double* d_length, uint32_t* d_n_path);
int vhp_planner_goal_paths(vhp_ctx* ctx, int solve, const int32_t* goals_qxy, int n_goals, int32_t* path_xy, uint32_t cap,
                           uint32_t* n_path, double* length, int32_t* path_status);
int vhp_planner_goal_paths_device(vhp_ctx* ctx, int solve, const int32_t* d_goals_qxy, int n_goals, int32_t* d_path_xy, uint32_t cap,
                                  uint32_t* d_n_path, double* d_length, int32_t* d_path_status);

/* Replaces raycasting() driven over all targets as benchmark() does (solver.cpp:226-232,
 * 267-290): a Bresenham ray from the source to every cell; a blocked cell met on the way
 * zeroes that cell and the target.  out: nx*ny doubles, 1 = visible (visibilityRayCasting_,
 * initialised to 1, solver.cpp:45).  Every write is a zero, so the union does not depend
 * on the order the rays are cast in and one thread per ray reproduces the reference. */
int vhp_raycast_all(vhp_ctx* ctx, int src_x, int src_y, double* out_host);

/* Replaces the same double loop (solver.cpp:226-232 over raycasting(), :267-290) for a batch of sources in one call, where
 * vhp_raycast_all takes one source, stores fp64 only and copies its field to the host every time.  Field i: nx*ny elements of `dtype`
 * (VHP_F64, VHP_F32 or VHP_U8, the same 0 / 1 values) at out + i*nx*ny, always packed ("field_stride" is not applied); exactly what the
 * reference leaves in visibilityRayCasting_ after a fresh reset() and that loop from source i -- for VHP_F64 the bytes of
 * vhp_raycast_all.  That is more than "is the target visible": the first blocked cell a ray meets is zeroed together with the ray's
 * target; a ray's own target is never tested, so a blocked cell in plain sight with nothing behind it (a blocked corner or border
 * cell) stays 1; a blocked source zeroes every cell; a 1 x 1 grid stays 1.
 * The kernels read the packed maps of vhp_set_map (x-major rays the column-packed copy, y-major rays the row-packed one), fill the
 * fields with ones and then store only zeros.  A source outside the grid leaves its field 0, the others are cast, and the call
 * returns VHP_ERR_SOURCE_OOB.  n_src = 0: VHP_OK, nothing launched.  No map set: VHP_ERR_NO_MAP; any other dtype: VHP_ERR_ARG.
 * vhp_last_elapsed_ms: fill plus kernel (of the last slice of ~1 GiB of fields the host form stages). */
int vhp_raycast_batch(vhp_ctx* ctx, const int32_t* src_xy, int n_src, int dtype, void* out_host);
/* Device-resident form: device pointers, asynchronous on the context's stream; d_out aligned to its element type (else VHP_ERR_ARG).
 * A rejected source's field is not written, and vhp_sync() reports VHP_ERR_SOURCE_OOB. */
int vhp_raycast_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, int n_src, int dtype, void* d_out);
/* The same loop run on a different environment per source: field i is cast from src_xy[2i..2i+1] on map map_idx[i] of the stack of
 * vhp_set_maps -- what vhp_set_map(that map) + vhp_raycast_batch gives.  Errors as vhp_sweep_maps_batch's: a source outside the grid or
 * a map index outside 0..n_maps-1 leaves its field 0 (device form: unwritten, reported by vhp_sync), the others are cast, the call
 * returns VHP_ERR_SOURCE_OOB; no stack set: VHP_ERR_NO_MAP. */
int vhp_raycast_maps_batch(vhp_ctx* ctx, const int32_t* src_xy, const int32_t* map_idx, int n_src, int dtype, void* out_host);
int vhp_raycast_maps_batch_device(vhp_ctx* ctx, const int32_t* d_src_xy, const int32_t* d_map_idx, int n_src, int dtype, void* d_out);

/* Replaces ONE call of raycasting(x0, y0, x1, y1) (solver.cpp:267-290), run for its answer only -- the reference offers the ray
 * through its side effect on visibilityRayCasting_ alone.  Pair i is pairs_xyxy[4i..4i+3] = (x0, y0, x1, y1) on the map of
 * vhp_set_map; hit_xy[2i..2i+1] is the first blocked cell the loop meets, or (-1, -1) where it reaches the target.  The target is
 * never tested; the start is, so a pair with equal ends is clear.  An endpoint outside the grid gives (-2, -2), and the call (for the
 * device form: vhp_sync) reports VHP_ERR_SOURCE_OOB with the other pairs answered.  n_pairs = 0: VHP_OK.  The single map only.  The
 * device form takes device pointers (4-byte aligned) and is asynchronous on the context's stream. */
int vhp_line_of_sight(vhp_ctx* ctx, const int32_t* pairs_xyxy, int n_pairs, int32_t* hit_xy);
int vhp_line_of_sight_device(vhp_ctx* ctx, const int32_t* d_pairs_xyxy, int n_pairs, int32_t* d_hit_xy);

/* MATLAB-flavoured variants.  The reference's MATLAB demos are a different algorithm from its C++ program:
 * MATLAB_code/visibility/getAccessibilityMap.m has an explicit diagonal rule (cell (i,i*1/fac) = alpha * its diagonal
 * predecessor), a decay `alpha` on every update, a curve factor `fac`, and sweeps every row and column.
 * vhp_sweep_batch_variant replaces getAccessibilityMap(alpha, 1, lightPos, 1-obstacle, ., fac) for a batch of sources
 * (fp64 fields, host buffers).  vhp_planner_solve_variant replaces the exploration loop of
 * MATLAB_code/c_sample_planner_solving_random_environments.m:100-171 over getAccessibilityMapPlanner.m (fac = 1):
 * first-lit labels at v >= threshold (0-based waypoint index, UINT64_MAX where none), min-max-scaled heuristic, stop when
 * the newest waypoint's own field sees the target; waypoints_xy holds 2*(max_iter+3) ints, waypoints_xy[0..1] = start.
 * Returns VHP_OK, VHP_ERR_MAX_ITER (the script itself has no bound) or VHP_ERR_NOTHING_LIT.
 * Parity: against a line-by-line CPU restatement of the .m files (oracle/vhp_oracle_matlab.cpp); MATLAB itself is not
 * available to the build, so these modes are unpinned against it.  Grid sides up to 4096. */
int vhp_sweep_batch_variant(vhp_ctx* ctx, const int32_t* src_xy, int n_src, double alpha, double fac, double* out_host);
int vhp_planner_solve_variant(vhp_ctx* ctx, int start_x, int start_y, int end_x, int end_y, double threshold, double alpha,
                              uint64_t max_iter, uint64_t* label, double* map_builder, double* local, int32_t* waypoints_xy,
                              uint32_t* n_waypoints);

/* computeVisibility() (solver.cpp:570-696) with the reference's local `offset` (:573; added to both operands of every c_,
 * :590-591 ... :686-687) exposed.  offset = 0 is the reference at HEAD and equals vhp_sweep_batch bit for bit (use that:
 * this entry point runs a plain anti-diagonal kernel, not the tuned ones).  It exists because the reference's published
 * Samples/SFMLstandAloneVisibility.png was rendered by a build with offset = 1; with it the library reproduces that
 * image.  fp64 fields, host buffers, cells the reference never writes are 0, grid sides up to 4096. */
int vhp_sweep_batch_offset(vhp_ctx* ctx, const int32_t* src_xy, int n_src, double offset, double* out_host);

/* Elapsed milliseconds of the most recent vhp_sweep_batch_device / planner call on the device.  How it is measured depends on
 * what the call launched:
 *  - the pool sweep and the latency sweep (vhp_last_sweep_kernel 3 and 4) time themselves: the launch's own kernels write
 *    timestamps of the device's constant-rate clock -- thread 0 of the launch's first kernel as its first act (the unit-ordering
 *    pre-kernel; every workgroup of a latency launch that has none), every workgroup of the sweep kernel when its wavefronts are
 *    done and their stores have landed -- and the time is the first of the first kernel's to the last workgroup's last.  Nothing is
 *    recorded on the stream for such a launch: it costs the launches around it no barrier packet.  The time holds no dispatch of
 *    either kernel, so it reads a few microseconds less than a pair of events around the same launch;
 *  - everything else -- the front sweep (vhp_last_sweep_kernel 1, and every vhp_sweep_maps_batch), the queue variant, ray casting
 *    and line of sight, the planner solves (one time around a whole solve), and a latency launch that would write more timestamps
 *    than two per CU of the device (a slot's size) -- is timed by two hipEvents recorded on the context stream around it, first
 *    kernel to last.  A library built with -DVHP_TIMING_STAMPS=0 times every launch this way.
 * The call blocks until that work has finished: it synchronises the stream the launch went out on (hipStreamSynchronize; for the
 * events, hipEventSynchronize) and, for a stamped launch, copies its timestamps to the host.  vhp_probe_stores and vhp_alloc_output
 * time their probes with the context's pair of events: after either of them there is nothing to report (VHP_ERR_ARG, "nothing timed
 * yet") until the next sweep or solve.  A launch whose timestamps cannot be read (VHP_ERR_HIP) did not finish or did not run.
 * The events carry no system-scope fence (hipEventDisableSystemFence): the call reports a time and is no point behind which the host
 * may read what the work wrote -- that is vhp_sync, hipStreamSynchronize or a copy on the stream. */
int vhp_last_elapsed_ms(vhp_ctx* ctx, float* ms);

/* Per-launch kernel timing for benchmarks.  vhp_timing(ctx, n), n >= 1, makes every following vhp_sweep_batch_device /
 * vhp_sweep_maps_batch_device call time what it launches -- the unit-ordering pre-kernel and the sweep kernel --; vhp_timing_collect
 * waits for the launches, writes up to `cap` durations in milliseconds (oldest first), returns their count in *n and clears the list.
 * vhp_timing(ctx, 0) switches it off.
 * A pool-sweep or latency-sweep launch is timed by the timestamps its own kernels write (vhp_last_elapsed_ms above: first stamp of
 * the launch's first kernel to last stamp of its last workgroup); no event is recorded for it, with vhp_timing on or off.  Its
 * timestamps go to one slot of a ring on the device that vhp_timing(ctx, n) sizes for n launches between two vhp_timing_collect
 * calls (n = 1: 64; the ring only grows, and only while no timed launch waits to be collected; it is allocated here, never inside a
 * launch).  The same slot serves vhp_last_elapsed_ms: for such a launch it and the launch's entry of vhp_timing_collect are the same
 * number, bit for bit.  A timed launch that finds the ring full is timed as every other kernel's launch is: by a pair of hipEvents
 * on the context stream around it (n > 1 also pre-creates n such pairs), inside the pair vhp_last_elapsed_ms reads.
 * vhp_timing_collect synchronises the stream(s) the stamped launches went out on (hipStreamSynchronize), copies the ring's slots to
 * the host in one copy (two where they wrap), and waits for the event pairs of the others (hipEventSynchronize).  A launch whose
 * time cannot be read -- timestamps of another launch in its slot, a pair that was never recorded -- is dropped and counted in the
 * error the call returns (VHP_ERR_HIP).  The events carry no system-scope fence (hipEventDisableSystemFence: recording one costs the
 * launches around it no cache write-back) and are for timing only: waiting for them orders no memory. */
int vhp_timing(vhp_ctx* ctx, int enable);  /* enable > 1: the ring's slots and the event pairs for that many timed launches */
int vhp_timing_collect(vhp_ctx* ctx, float* ms_out, int cap, int* n);

/* Launch-shape overrides for tuning and for parity tests that must reach every compiled shape
 * (0 / -1 = automatic, the default).  Keys: "rows_per_lane" (1, 2, 4), "strips" (1..8 wavefront
 * strips per octant), "multi_round" (1 = force the multi-round build), "slide" (0 / 1: y-major
 * column grid slid onto 128-byte lines), "pack" (1 = pack short quadrants), "lat_workgroups" (1, 2, 4, 8:
 * workgroups per octant of a latency-sweep launch; 0: one up to 1024 cells a side, two up to 2048, four up to 4096, eight beyond,
 * halved until the launch is resident at once), "kernel" (1 = front
 * sweep, 3 = pool sweep, 4 = latency sweep; 2 was the streaming sweep, retired in round 4 and refused),
 * "pool_contexts" (1..16: units a workgroup of the pool sweep holds
 * at once), "pool_static_round" (0: every unit of a pool-sweep launch is pulled from its queue; 1: the first unit of
 * every context is handed out by workgroup index; 2, the default: ... and a workgroup's second unit counts down from the end of the
 * round, so that the longest units share their CU with the shortest of the round), "field_stride" (elements from one field of a DEVICE-pointer batch to the next;
 * 0 = nx * ny, packed; a value below nx * ny makes vhp_sweep_batch_device fail with VHP_ERR_ARG; the host-buffer entry points
 * ignore it -- their results are packed --, the queue variant refuses it, and vhp_set_map resets it to 0),
 * "alloc_budget_pct" (vhp_alloc_output below), "planner_batch_group" (0 automatic, 1..32: queries per group of
 * vhp_planner_solve_batch at most).  The
 * results never depend on these; only the schedule (and, with field_stride, the placement of the fields) does. */
int vhp_set_option(vhp_ctx* ctx, const char* key, long long value);
/* Which kernel the last batch sweep of this context launched: 1 = front sweep (vhp_sweep_fronts),
 * 3 = pool sweep (vhp_pool_sweep), 4 = latency sweep
 * (vhp_lat_sweep; vhp_lat_maps_sweep on a stack of maps), 0 = none yet.  For benchmarks and profiles. */
int vhp_last_sweep_kernel(const vhp_ctx* ctx);

/* The max-union of a batch of fields and the source that attains it, on the device: best[c] = max over k of field k at cell c,
 * arg[c] = first_index + the lowest k that attains it (a sequential max-union that replaces on strict improvement only) -- the
 * reference's union, src/visibilityBasedSolver.cpp:417-418 (visibility_global_ = max(visibility_, visibility_global_)), over a
 * whole batch at once, with the label the planner derives from it (:419-423).  What a batch sharded over several devices exchanges
 * instead of its fields (option 2: one union field and one label field per device).  d_fields: n_fields fields of nx * ny
 * elements of `dtype` (the map's grid; "field_stride" elements apart as in vhp_sweep_batch_device); d_best: nx * ny elements of
 * dtype; d_arg: nx * ny int32.  n_fields = 0: best = -1, arg = INT32_MAX everywhere.  One pass over the fields, no temporaries;
 * asynchronous on the context's stream.  Not timed: vhp_last_elapsed_ms still reports the sweep or planner call before it.
 * vhp_union_partials_device: the same reduction over n_parts PARTIAL results -- d_bests: n_parts packed union fields, d_args: their
 * n_parts packed label fields (e.g. the partials of all devices after an all-gather); a tie goes to the lowest label. */
int vhp_union_fields_device(vhp_ctx* ctx, const void* d_fields, int n_fields, int dtype, int first_index, void* d_best, int32_t* d_arg);
int vhp_union_partials_device(vhp_ctx* ctx, const void* d_bests, const int32_t* d_args, int n_parts, int dtype, void* d_best, int32_t* d_arg);

/* A measurement aid, not part of the reference's surface (it has no device memory): the rate at which the memory behind a
 * device buffer takes two store patterns of a sweep launch, in TB/s of bytes stored -- 1 KB row pieces in many concurrent
 * streams, (a) every piece on the 128-byte line grid, (b) every other piece half a line off it, so that two lines per piece
 * are written in halves by different wavefronts at different times, with PLAIN stores.  The same physical memory answers (a)
 * with 4.9-5.0 or 5.9-6.1 and (b) with 3.6-3.7 or 5.2-5.4 depending on where the allocation landed;
 * bench.py reports both for the buffer it timed so that a result can be read against the state of its memory; vhp_alloc_output
 * (below) places a result buffer by it.  d_buf: 128-byte aligned, at least 128 MB; its contents are overwritten with zeros
 * (up to 16 GB of it are used).  Blocks until done. */
int vhp_probe_stores(vhp_ctx* ctx, void* d_buf, unsigned long long bytes, float* whole_lines_TBps, float* split_lines_TBps);

/* Device memory for results, placed by the library (the reference has no device memory; a maintainer's binding allocates its
 * result fields with this instead of hipMalloc).  The memory behind an allocation is of a faster or a slower kind, and no allocation
 * API chooses (a launch of 256 fields at 1000^2 takes 15-20 % longer on the one than on the other): up to
 * max_candidates allocations of `bytes` are made, each is probed (vhp_probe_stores; from 128 MB up), the one whose two rates add up
 * highest is kept, the others are freed.  BEST EFFORT: where the fast kind is rare the keeper is merely the best of what was tried.
 * The search is a guest on the device: the candidates -- all held until the choice is made, a freed one would be handed out
 * again -- stay within 25 % of the device memory that is free when the search starts (vhp_set_option "alloc_budget_pct", 1..90)
 * and within 64; it ends on the first buffer of the fast kind and after 8 candidates in a row that are no better than the best so
 * far.  While it runs, other users of the device see that much less free memory.  d_buf: 256-byte aligned, contents undefined.
 * whole_lines_TBps / split_lines_TBps (may be NULL): the probe's rates of the buffer kept (0 below 128 MB); n_tried (may be NULL):
 * allocations made.  Blocks; a one-off cost of 5-10 ms per candidate (vhp_alloc_output_cost tells what the last search took).
 * Buffers still allocated when the context is destroyed are freed with it. */
int vhp_alloc_output(vhp_ctx* ctx, unsigned long long bytes, int max_candidates, void** d_buf, float* whole_lines_TBps,
                     float* split_lines_TBps, int* n_tried);
/* What the last vhp_alloc_output of this context cost: wall-clock milliseconds of the search, and the device memory its
 * candidates held at the peak (bytes).  Either pointer may be NULL. */
int vhp_alloc_output_cost(const vhp_ctx* ctx, double* search_ms, unsigned long long* peak_bytes);
int vhp_free_output(vhp_ctx* ctx, void* d_buf);

/* ---- several devices of one node (the reference is one thread on one CPU and has nothing to replace here) ----
 * The sources of a batch are independent, so a batch shards over devices with no exchange step: device d of n sweeps the
 * block vhp_multi_shard_bounds(n_src, n, d) of the sources into its own buffer.  vhp_multi_create makes one context per listed
 * device (an ordinal may be listed twice: two contexts on one device), each with a stream of its own; vhp_multi_set_map gives
 * every device the map; vhp_multi_sweep_batch uploads the shards' sources, launches every device's sweep before it waits for
 * any, and returns the first device-side status that is not VHP_OK (d_out_per_device[d]: device memory ON device d for its
 * shard's fields, packed; NULL allowed where the shard is empty; on an error of device d the sweeps already enqueued on the
 * devices before it are waited for before the call returns); vhp_multi_allgather_fields then lands all n_src fields in source
 * order in d_all_per_device[d] on every device.  By default by direct peer copies: xGMI is point to point, every pair of devices
 * has a link of its own, and every (destination, source) pair has a STREAM of its own ("lane" k of device `to` carries the copy
 * from device (to + k) mod N), so the N - 1 inbound copies of a device are in flight together, one per link, and in round k no
 * two destinations pull from one source.  vhp_multi_allgather_plan returns that enqueue plan as data -- (to, from, lane, first
 * and one-past-last source of the piece) per copy, in enqueue order, up to `cap` entries; its return value is the number of
 * copies; host arithmetic only.  vhp_multi_use_rccl(m, 1) switches to RCCL instead (ncclAllGather on a single-process
 * communicator over the listed devices, one group call; librccl is loaded at run time; distinct devices only -- VHP_ERR_ARG when
 * an ordinal is listed twice --; a batch that does not divide by the number of devices still takes the peer copies).  The planner
 * does not shard (pivot k + 1 needs the union after pivot k): use vhp_multi_context(m, d) for replicas.  (torch.distributed /
 * RCCL form of the same: dist.py.)  Not thread-safe; every call restores the caller's current device.  Never run across devices
 * so far (no multi-GPU node was available): correct by construction, tested with one ordinal listed several times. */
typedef struct vhp_multi vhp_multi;
int vhp_multi_create(const int* device_ordinals, int n_devices, vhp_multi** out);
int vhp_multi_destroy(vhp_multi* m);
const char* vhp_multi_last_error(const vhp_multi* m);
int vhp_multi_devices(const vhp_multi* m);
vhp_ctx* vhp_multi_context(vhp_multi* m, int d);
void vhp_multi_shard_bounds(int n_src, int n_devices, int d, int* lo, int* hi);
int vhp_multi_set_map(vhp_multi* m, const uint8_t* occ_rowmajor, int nx, int ny);
int vhp_multi_sweep_batch(vhp_multi* m, const int32_t* src_xy, int n_src, int variant, int dtype, void* const* d_out_per_device);
int vhp_multi_allgather_fields(vhp_multi* m, int n_src, int dtype, void* const* d_shard_per_device, void* const* d_all_per_device);
int vhp_multi_allgather_plan(int n_src, int n_devices, int* to, int* from, int* lane, int* lo, int* hi, int cap);
int vhp_multi_use_rccl(vhp_multi* m, int enable);
/* The max-union of ALL n_src fields of a sharded batch and the source that attains it (vhp_union_fields_device), on every device:
 * each device reduces its own shard (one pass over its fields), the N partial results -- one union field and one label field per
 * device, whatever the batch -- are exchanged (peer copies on the lanes of vhp_multi_allgather_plan, or ncclAllGather after
 * vhp_multi_use_rccl), and every device merges them (vhp_union_partials_device; a tie goes to the lowest source index).  SURVEY 8e,
 * option 2: what the planner needs of a batch is this, not the fields (at BASELINE config 5: 0.2 GB per device instead of 137).
 * d_shard_per_device[d]: device d's fields as vhp_multi_sweep_batch left them; d_best_per_device[d]: nx * ny elements of dtype on
 * device d; d_arg_per_device[d]: nx * ny int32 there.  Blocks.  Like the rest of vhp_multi_*: NEVER RUN ACROSS DEVICES in this
 * repository's test environment (one GPU; the tests list its ordinal twice). */
int vhp_multi_union_fields(vhp_multi* m, int n_src, int dtype, void* const* d_shard_per_device, void* const* d_best_per_device,
                           int32_t* const* d_arg_per_device);

/* Library / build identification: "vhp-hip <version> gfx950". */
const char* vhp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VHP_H */
