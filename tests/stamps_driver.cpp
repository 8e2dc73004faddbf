// stamps_driver.cpp -- csrc/vhp_stamps.hpp (the bookkeeping of the timestamps a sweep launch writes from inside its kernels) on the
// CPU, for tests/test_stamps.py.  One request per line on stdin, one line of answer each:
//   sizes G                     -> slot_entries(G) slot_bytes(G)
//   ring N G                    -> 1 / 0 (resized or not), then: slots groups live bytes
//   take | untake | release K   -> the slot taken (-1: full) / live
//   oldest                      -> the oldest slot that is out, -1: none
//   runs                        -> the runs to copy, "first:count" each, "-": none
//   fits NB NE                  -> 1 / 0
//   offset S                    -> slot S's first entry
//   ms TICKS KHZ                -> the time, %.9g
//   reduce KHZ NB NE TAG t:tag ...   -> "ok ms" of a slot with the NB + NE entries given (a missing entry: leave it out, 0:0 is used)
//   timed N G KHZ L             -> a context in small: a device array for a ring of N slots, L timed launches of G workgroups and a
//                                  pre-kernel (the launch writes its entries the moment it is made: begin at 1000 * k, ends up to
//                                  1000 * k + 500 + g), one collect, then vhp_last_elapsed_ms's answer, then a second collect.
//                                  -> per launch "s<slot>" or "ev"; "| collect" the stamped times in order; "| last <state> <ms>";
//                                  "| collect2" count
// Exit 0 if every request was well-formed.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vhp_stamps.hpp"

using namespace vhp::stamps;

static int timed_scenario(int n, int groups, int khz, int launches) {
  Ring ring;
  ring.resize(n, groups);
  std::vector<Entry> dev(ring.bytes() / sizeof(Entry));   // exactly the array's size: a slot past it is a heap overflow
  std::vector<Entry> host(dev.size(), Entry{0, 0});
  std::vector<Launch> out;   // the timed launches, oldest first; slot -1: an event pair
  Last last;
  unsigned long long epoch = 0x5A17000000000000ull;
  for (int k = 0; k < launches; ++k) {
    Launch l;
    if (ring.fits(1, groups)) l.slot = ring.take();
    l.n_begin = 1;
    l.n_end = groups;
    l.tag = ++epoch;
    if (l.stamped()) {
      Entry* s = dev.data() + ring.slot_offset(l.slot);
      s[0] = {1000ull * k, l.tag};
      for (int g = 0; g < groups; ++g) s[1 + g] = {1000ull * k + 500 + g, l.tag};
      last.stamps(l);
    } else {
      last.events();
    }
    out.push_back(l);
    std::printf("%s ", l.stamped() ? ("s" + std::to_string(l.slot)).c_str() : "ev");
  }
  // collect: the runs copied, every stamped launch reduced, the slots given back
  int first[2], count[2];
  const int n_runs = ring.runs(first, count);
  for (int r = 0; r < n_runs; ++r) {
    const size_t at = ring.slot_offset(first[r]);
    std::memcpy(host.data() + at, dev.data() + at, (size_t)count[r] * slot_bytes(ring.groups()));
  }
  std::printf("| collect");
  int n_stamped = 0;
  for (const Launch& l : out) {
    if (!l.stamped()) continue;
    ++n_stamped;
    const Time t = reduce(host.data() + ring.slot_offset(l.slot), l, khz);
    last.read(l.tag, t);
    std::printf(" %d:%.9g", (int)t.ok, (double)t.ms);
  }
  ring.release(n_stamped);
  out.clear();
  std::printf(" | last %d %.9g", (int)last.state, last.state == Last::kRead ? (double)last.time.ms : -1.0);
  std::printf(" | collect2 %d live %d\n", (int)out.size(), ring.live());
  return 0;
}

int main() {
  Ring ring;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "sizes") {
      int g;
      if (!(in >> g)) return 2;
      std::printf("%zu %zu\n", slot_entries(g), slot_bytes(g));
    } else if (cmd == "ring") {
      int n, g;
      if (!(in >> n >> g)) return 2;
      const bool ok = ring.resize(n, g);
      std::printf("%d %d %d %d %zu\n", (int)ok, ring.slots(), ring.groups(), ring.live(), ring.bytes());
    } else if (cmd == "take") {
      const int slot = ring.take();
      std::printf("%d %d\n", slot, ring.live());
    } else if (cmd == "untake") {
      ring.untake();
      std::printf("%d\n", ring.live());
    } else if (cmd == "release") {
      int k;
      if (!(in >> k)) return 2;
      ring.release(k);
      std::printf("%d\n", ring.live());
    } else if (cmd == "oldest") {
      std::printf("%d\n", ring.oldest());
    } else if (cmd == "runs") {
      int first[2], count[2];
      const int n = ring.runs(first, count);
      if (n == 0) std::printf("-");
      for (int r = 0; r < n; ++r) std::printf("%s%d:%d", r ? " " : "", first[r], count[r]);
      std::printf("\n");
    } else if (cmd == "fits") {
      int nb, ne;
      if (!(in >> nb >> ne)) return 2;
      std::printf("%d\n", (int)ring.fits(nb, ne));
    } else if (cmd == "offset") {
      int s;
      if (!(in >> s)) return 2;
      std::printf("%zu\n", ring.slot_offset(s));
    } else if (cmd == "ms") {
      unsigned long long t;
      int khz;
      if (!(in >> t >> khz)) return 2;
      std::printf("%.9g\n", (double)ticks_to_ms(t, khz));
    } else if (cmd == "reduce") {
      int khz;
      Launch l;
      l.slot = 0;
      if (!(in >> khz >> l.n_begin >> l.n_end >> l.tag)) return 2;
      std::vector<Entry> slot((size_t)(l.n_begin > 0 ? l.n_begin : 0) + (size_t)(l.n_end > 0 ? l.n_end : 0), Entry{0, 0});
      std::string e;
      for (size_t k = 0; k < slot.size() && (in >> e); ++k) {
        const size_t colon = e.find(':');
        if (colon == std::string::npos) return 2;
        slot[k] = {std::stoull(e.substr(0, colon)), std::stoull(e.substr(colon + 1))};
      }
      const Time t = reduce(slot.data(), l, khz);
      std::printf("%d %.9g\n", (int)t.ok, (double)t.ms);
    } else if (cmd == "timed") {
      int n, g, khz, launches;
      if (!(in >> n >> g >> khz >> launches)) return 2;
      timed_scenario(n, g, khz, launches);
    } else {
      return 2;
    }
  }
  return 0;
}
