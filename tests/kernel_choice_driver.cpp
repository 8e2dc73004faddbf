// Reads launches from stdin, one per line -- nx ny n_src n_cus f64 kernel rows_per_lane strips multi slide pack lat_ok pool_ok
// lat_scratch_fits -- and prints vhp::plan_sweep's answer for each as five digits: kernel R W multi slide.
// Built by tests/test_kernel_choice.py with the host compiler against csrc/vhp_choice.hpp.
#include <cstdio>

#include "vhp_choice.hpp"

int main() {
  vhp::ChoiceIn in;
  int f64, lat_ok, pool_ok, fits;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &in.nx, &in.ny, &in.n_src, &in.n_cus, &f64, &in.opt.kernel,
                    &in.opt.rows_per_lane, &in.opt.strips, &in.opt.multi, &in.opt.slide, &in.opt.pack, &lat_ok, &pool_ok, &fits) == 14) {
    in.f64 = f64 != 0;
    in.lat_ok = lat_ok != 0;
    in.pool_ok = pool_ok != 0;
    in.lat_scratch_fits = fits != 0;
    const vhp::SweepPlan p = vhp::plan_sweep(in);
    std::printf("%d%d%d%d%d\n", p.kernel, p.R, p.W, p.multi ? 1 : 0, p.slide);
  }
  return 0;
}
