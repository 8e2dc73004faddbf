// vhp_lat_maps_sim.cpp -- CPU simulator of the latency sweep on a stack of maps (vhp_lat.hip vhp_lat_maps_sweep).  TEST
// INFRASTRUCTURE ONLY.
//
// The band sweep's own source (csrc/vhp_band.hpp BandWorker with its STACK flag) under the scheduler of vhp_pool_sim.cpp, which this
// file compiles in as it is: the same coroutines, policies, NaN-poisoned LDS and scratch lines, and deadlock detection.  The stack is
// laid out as vhp_set_maps lays it out -- every map's row- and column-packed words one after the other -- and its diagonal maps are
// built as the first planner batch on it builds them (vhp_lat.hip vhp_pack_diag_stack): word by word from the row-packed words with
// diag_word_from_rows.  Each worker starts from map 0's copies and moves itself to its source's map in BandWorker::run, as on the GPU.
//
// Only tests/ loads this library (tests/lat_maps_sim.py).
#include "vhp_pool_sim.cpp"

namespace {

// the stack that the next run's workers sweep (set before run_lat_t starts them)
struct SimStack {
  std::vector<uint64_t> rows, cols, diag;
  LatMapStack st;
};
SimStack g_stack;

// BandWorker in its STACK build, pointed at the stack: what vhp_lat_maps_sweep does with its kernel arguments
template <typename OutT, bool ODD, bool MULTI>
struct StackWorker : BandWorker<OutT, ODD, MULTI, true> {
  void init(const LatArgs<OutT>& a, double* lds, const Layout& L, int w) {
    BandWorker<OutT, ODD, MULTI, true>::init(a, lds, L, w);
    this->a.m.rows = g_stack.rows.data();
    this->a.m.cols = g_stack.cols.data();
    this->a.dmap = g_stack.diag.data();
    this->stk = g_stack.st;
  }
};

// the stack of n_maps byte maps at occ (map k at occ + k * nx * ny)
void build_stack(const uint8_t* occ, int n_maps, int nx, int ny, SimStack& s) {
  s.rows.clear();
  s.cols.clear();
  for (int k = 0; k < n_maps; ++k) {
    HostMap h;
    build_map(occ + (size_t)k * nx * ny, nx, ny, h);
    s.rows.insert(s.rows.end(), h.rows.begin(), h.rows.end());
    s.cols.insert(s.cols.end(), h.cols.begin(), h.cols.end());
  }
  const int wpr = (nx + 63) / 64 + 2, wpc = (ny + 63) / 64 + 2;
  const size_t words = DiagMaps::words(nx, ny);
  s.diag.assign(words * n_maps, ~0ull);   // (every word is written below, the pad words included)
  for (int k = 0; k < n_maps; ++k)
    for (size_t w = 0; w < words; ++w) s.diag[(size_t)k * words + w] = diag_word_from_rows(s.rows.data() + (size_t)k * ny * wpr, wpr, nx, ny, w);
  s.st.map_idx = nullptr;
  s.st.n_maps = n_maps;
  s.st.rows_stride = (long long)ny * wpr;
  s.st.cols_stride = (long long)nx * wpc;
  s.st.diag_stride = (long long)words;
}

}  // namespace

extern "C" {

// Fields [n_src, ny, nx] (fp64) of the latency sweep of source s on map map_idx[s] of the stack: W sweepers per workgroup, the
// workgroups per unit of vhp_sim_set_lat_halves (1: the one-workgroup build, 2: the MULTI build); stats as vhp_sim_band_sweep's.
int vhp_sim_lat_maps_sweep(const uint8_t* occ, int n_maps, int nx, int ny, const int32_t* src, const int32_t* map_idx, int n_src, void* out,
                           int W, int policy, unsigned seed, long long* stats) {
  if (n_maps < 1 || nx < 1 || ny < 1 || n_src < 0 || W < 1) return 1;
  build_stack(occ, n_maps, nx, ny, g_stack);
  g_stack.st.map_idx = map_idx;
  double* o = static_cast<double*>(out);
  const bool odd = lat_needs_odd<double>(nx, (long long)nx * ny, o);
  // (map 0 gives run_lat_t the grid and the reciprocal table; the workers read the stack)
  if (g_lat_halves > 1)
    return odd ? run_lat_t<double, true, StackWorker<double, true, true>>(occ, nx, ny, src, n_src, o, W, policy, seed, stats)
               : run_lat_t<double, false, StackWorker<double, false, true>>(occ, nx, ny, src, n_src, o, W, policy, seed, stats);
  return odd ? run_lat_t<double, true, StackWorker<double, true, false>>(occ, nx, ny, src, n_src, o, W, policy, seed, stats)
             : run_lat_t<double, false, StackWorker<double, false, false>>(occ, nx, ny, src, n_src, o, W, policy, seed, stats);
}

// The stack's diagonal maps two ways, words(nx, ny) words per map: as vhp_pack_diag_stack builds them from the row-packed words
// (from_rows), and as vhp_pack_diag builds one map's from its bytes (from_bytes: the simulator's build_map).
int vhp_sim_stack_diag_words(const uint8_t* occ, int n_maps, int nx, int ny, uint64_t* from_rows, uint64_t* from_bytes) {
  if (n_maps < 1 || nx < 1 || ny < 1) return 1;
  SimStack s;
  build_stack(occ, n_maps, nx, ny, s);
  const size_t words = DiagMaps::words(nx, ny);
  std::copy(s.diag.begin(), s.diag.end(), from_rows);
  for (int k = 0; k < n_maps; ++k) {
    HostMap h;
    build_map(occ + (size_t)k * nx * ny, nx, ny, h);
    std::copy(h.diag.begin(), h.diag.end(), from_bytes + (size_t)k * words);
  }
  return 0;
}

unsigned long long vhp_sim_diag_words(int nx, int ny) { return DiagMaps::words(nx, ny); }

}  // extern "C"
