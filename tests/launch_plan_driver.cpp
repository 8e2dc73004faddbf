// Reads launches from stdin, one per line, and prints the launch plan of each (csrc/vhp_launch_plan.hpp) as one word:
//   pool NX NY N_SRC N_CUS ANYW contexts claim_ahead heads tail_pct early_ctx late_pct busy_cap static_round
//     -> ok,n_ctx,waves,lds_bytes,n_head,tail_limit,early_ctx,late_after,claim_ahead,busy_cap,static_round,static_snake,queue0
//        (queue0 as head+tail: its low and its high word)
//   lat NX NY N_SRC N_CUS ODD ASKED d_lat_order pivot_rec src_index slot_base map_idx planner_dev
//     -> ok,odd,halves,lds_bytes,use_order_kernel
//   grid NX NY
//     -> pool_supported,lat_supported
// Built by tests/test_launch_plans.py with the host compiler and -DVHP_SIM, once plain and once under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>

#include "vhp_launch_plan.hpp"

int main() {
  char what[8];
  int nx, ny, n_src, n_cus;
  while (std::scanf("%7s %d %d", what, &nx, &ny) == 3) {
    if (!std::strcmp(what, "grid")) {
      std::printf("%d,%d\n", vhp::pool_supported(nx, ny) ? 1 : 0, vhp::lat_supported(nx, ny) ? 1 : 0);
    } else if (!std::strcmp(what, "pool")) {
      int anyw;
      vhp::PoolOpts o;
      if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &n_src, &n_cus, &anyw, &o.contexts, &o.claim_ahead, &o.heads, &o.tail_pct, &o.early_ctx,
                     &o.late_pct, &o.busy_cap, &o.static_round) != 11) return 2;
      const vhp::PoolPlan p = vhp::plan_pool(nx, ny, n_src, n_cus, anyw != 0, o);
      std::printf("%d,%d,%d,%zu,%d,%d,%d,%d,%d,%d,%d,%d,%llu+%llu\n", p.ok ? 1 : 0, p.n_ctx, p.waves, p.lds_bytes, p.n_head, p.tail_limit, p.early_ctx,
                  p.late_after, p.claim_ahead, p.busy_cap, p.static_round ? 1 : 0, p.static_snake ? 1 : 0, p.queue0 & 0xffffffffull, p.queue0 >> 32);
    } else if (!std::strcmp(what, "lat")) {
      int odd, asked, f[6];
      if (std::scanf("%d %d %d %d %d %d %d %d %d %d", &n_src, &n_cus, &odd, &asked, &f[0], &f[1], &f[2], &f[3], &f[4], &f[5]) != 10) return 2;
      const vhp::LatPlan p = vhp::plan_lat(nx, ny, n_src, n_cus, odd != 0, asked, {f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0, f[4] != 0, f[5] != 0});
      std::printf("%d,%d,%d,%zu,%d\n", p.ok ? 1 : 0, p.odd ? 1 : 0, p.halves, p.lds_bytes, p.use_order_kernel ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
