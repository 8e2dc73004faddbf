// vhp_raycast.hpp -- raycasting() (reference src/visibilityBasedSolver.cpp:267-290) for batches of sources: the ray walk, the packed-map
// reader and the launch decisions, written once for the device and for the host compiler (no HIP types: tests/raycast_driver.cpp builds
// them with g++).  vhp_raycast.hip.h holds the kernels around them.
//
// The reference's ray from (x0, y0) to (x1, y1):
//   err = dx - dy; while not at the target { test the cell; e2 = 2 err; if (e2 > -dy) { err -= dy; x += sx; } if (e2 < dx) { err += dx; y += sy; } }
// tests every cell from the start up to, not including, the target.  Its loop takes exactly max(dx, dy) iterations and the coordinate
// with the longer side advances in each one (tests/test_raycast_cpu.py re-checks that for every dx, dy <= 512 and for all of dx = 4095
// and 8191), so the walk here is a COUNTED loop of that many steps with the reference's own err arithmetic: it ends whatever it is fed.
// The arithmetic is symmetric in the two axes (swap x and y: err changes sign and the two tests change places), so the walk runs on
// (major, minor) coordinates -- major is x where dx >= dy -- and reads the map that is packed ALONG THE MINOR axis: at step k every
// x-major ray of a source is in column x0 +- k, so the 64 targets of a wavefront ask for the same one or two words of `cols`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHP_RAY_HD __host__ __device__
#else
#define VHP_RAY_HD
#endif

namespace vhp {

// The packed copies of one map (vhp_pack_rows / vhp_pack_cols; 1 = free): bit x & 63 of rows[y * wpr + 1 + (x >> 6)] and bit y & 63 of
// cols[x * wpc + 1 + (y >> 6)] are cell (x, y); word 0 and the last word of a line are pads.  Map k of a stack: both pointers moved
// by k times MapStack's strides.
struct PackedOcc {
  const uint64_t* rows;
  const uint64_t* cols;
  int wpr, wpc;
  // the lines a ray reads: those of its major coordinate, packed along its minor one
  struct View {
    const uint64_t* line;
    int words;
    VHP_RAY_HD bool free_at(int major, int minor) const { return (line[(unsigned)(major * words + 1 + (minor >> 6))] >> (minor & 63)) & 1; }  // (below 8192 * 131 words)
  };
  VHP_RAY_HD View view(bool x_major) const { return x_major ? View{cols, wpc} : View{rows, wpr}; }
};

// One ray: a, b its major and minor coordinate, n = max(dx, dy) its steps.
struct Ray {
  int a, b, sa, sb, da, db, err, n;
  bool x_major;
  VHP_RAY_HD int x() const { return x_major ? a : b; }
  VHP_RAY_HD int y() const { return x_major ? b : a; }
};

VHP_RAY_HD inline Ray ray_begin(int x0, int y0, int x1, int y1) {
  const int dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
  const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
  Ray r;
  r.x_major = dx >= dy;
  r.a = r.x_major ? x0 : y0;
  r.b = r.x_major ? y0 : x0;
  r.sa = r.x_major ? sx : sy;
  r.sb = r.x_major ? sy : sx;
  r.da = r.x_major ? dx : dy;
  r.db = r.x_major ? dy : dx;
  r.err = r.da - r.db;
  r.n = r.da;
  return r;
}

// One iteration of the reference's loop behind its occupancy test.  Its first test, e2 > -db, always holds on the major axis (that is
// the statement above: the major coordinate advances in every iteration), so the step is taken without it; the driver walks every ray
// it checks beside the reference's loop, cell by cell.
VHP_RAY_HD inline void ray_step(Ray& r) {
  const int e2 = 2 * r.err;
  r.err -= r.db;
  r.a += r.sa;
  if (e2 < r.da) { r.err += r.da; r.b += r.sb; }
}

struct RayProbe {
  int a, b;
  bool blocked;
};
// one step of the ray: where it stands and whether that cell is blocked (the caller stays inside the ray's n steps)
template <typename View>
VHP_RAY_HD inline RayProbe ray_probe(const View& v, Ray& r) {
  const RayProbe p{r.a, r.b, !v.free_at(r.a, r.b)};
  ray_step(r);
  return p;
}

// The reference's raycasting(x0, y0, x1, y1) for its answer: true and the first blocked cell the loop meets in (*hit_x, *hit_y), or
// false where it reaches the target.  The start is tested, the target never; equal ends are clear.  Both ends inside the grid.
// Four steps per exit test while four are left -- four independent, unconditional loads in flight, the first blocked one of them
// taken --, then the last one to three steps one by one.  No step reads behind the ray's last cell.
template <typename Occ>
VHP_RAY_HD inline bool ray_walk(const Occ& occ, int x0, int y0, int x1, int y1, int* hit_x, int* hit_y) {
  Ray r = ray_begin(x0, y0, x1, y1);
  const auto v = occ.view(r.x_major);
  int k = 0;
  for (; k + 4 <= r.n; k += 4) {
    const RayProbe p0 = ray_probe(v, r), p1 = ray_probe(v, r), p2 = ray_probe(v, r), p3 = ray_probe(v, r);
    if (p0.blocked | p1.blocked | p2.blocked | p3.blocked) {
      const RayProbe h = p0.blocked ? p0 : p1.blocked ? p1 : p2.blocked ? p2 : p3;
      *hit_x = r.x_major ? h.a : h.b;
      *hit_y = r.x_major ? h.b : h.a;
      return true;
    }
  }
  for (; k < r.n; ++k) {
    const RayProbe h = ray_probe(v, r);
    if (h.blocked) {
      *hit_x = r.x_major ? h.a : h.b;
      *hit_y = r.x_major ? h.b : h.a;
      return true;
    }
  }
  return false;
}

// ---- the launch of the field kernels (vhp_raycast_fill, vhp_raycast_fields) -------------------------------------------------------
// A workgroup of kRaycastBlock threads takes one tile of kRaycastBlock consecutive cells (x fastest: a wavefront is 64 consecutive x
// of a target row where the width allows) of one source; the grid is (tiles, sources).  gridDim.y ends at 65535: workgroup row y takes
// the sources y, y + gridDim.y, ... (raycast_for_sources), so any batch is one launch and needs no chunking.
constexpr int kRaycastBlock = 256;
constexpr int kRaycastMaxGridY = 65535;

struct RaycastPlan {
  unsigned block, tiles, grid_y;  // grid_y = 0: nothing to launch
};

inline RaycastPlan plan_raycast(long long cells, int n_src) {
  RaycastPlan p;
  p.block = kRaycastBlock;
  p.tiles = (unsigned)((cells + kRaycastBlock - 1) / kRaycastBlock);  // (8192^2 cells: 262144 tiles)
  p.grid_y = (unsigned)(n_src < kRaycastMaxGridY ? (n_src > 0 ? n_src : 0) : kRaycastMaxGridY);
  return p;
}

// the sources of workgroup row block_y
template <typename F>
VHP_RAY_HD inline void raycast_for_sources(unsigned block_y, unsigned grid_y, int n_src, F f) {
  for (long long s = block_y; s < n_src; s += grid_y) f((int)s);
}

// Whether source s is cast: inside the grid, and on a stack its map index inside the stack (map_idx null: the single map).
VHP_RAY_HD inline bool raycast_source_ok(const int32_t* src_xy, const int32_t* map_idx, int s, int nx, int ny, int n_maps) {
  const int x = src_xy[2 * (size_t)s], y = src_xy[2 * (size_t)s + 1];
  if (x < 0 || y < 0 || x >= nx || y >= ny) return false;
  return !map_idx || (map_idx[s] >= 0 && map_idx[s] < n_maps);
}

}  // namespace vhp
