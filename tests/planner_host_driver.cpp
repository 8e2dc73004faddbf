// Reads one request per line from stdin and prints csrc/vhp_planner_host.hpp's answer on one line:
//   check nx ny sx sy ex ey occ_start occ_end  ->  planner_check_query's code, then its message ("-" when the query passes)
//   status code                                ->  planner_status_message's message ("-" when there is none)
//   scale nx ny                                ->  planner_scale, as a hexadecimal float (every bit)
//   pivots max_iter extra                      ->  planner_pivot_ints
// Built by tests/test_planner_host.py with the host compiler alone.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "vhp_planner_host.hpp"

int main() {
  char what[16];
  while (std::scanf("%15s", what) == 1) {
    if (!std::strcmp(what, "check")) {
      int nx, ny, sx, sy, ex, ey, os, oe;
      if (std::scanf("%d %d %d %d %d %d %d %d", &nx, &ny, &sx, &sy, &ex, &ey, &os, &oe) != 8) return 2;
      const vhp::QueryCheck c = vhp::planner_check_query(nx, ny, sx, sy, ex, ey, (uint8_t)os, (uint8_t)oe);
      std::printf("%d %s\n", c.code, c.msg ? c.msg : "-");
    } else if (!std::strcmp(what, "status")) {
      int code;
      if (std::scanf("%d", &code) != 1) return 2;
      const char* m = vhp::planner_status_message(code);
      std::printf("%s\n", m ? m : "-");
    } else if (!std::strcmp(what, "scale")) {
      int nx, ny;
      if (std::scanf("%d %d", &nx, &ny) != 2) return 2;
      std::printf("%a\n", vhp::planner_scale(nx, ny));
    } else if (!std::strcmp(what, "pivots")) {
      uint64_t max_iter;
      int extra;
      if (std::scanf("%" SCNu64 " %d", &max_iter, &extra) != 2) return 2;
      std::printf("%zu\n", vhp::planner_pivot_ints(max_iter, extra));
    } else {
      return 2;
    }
  }
  return 0;
}
