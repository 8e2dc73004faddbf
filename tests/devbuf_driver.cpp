// Drives csrc/vhp_devbuf.hpp's Buf over an allocator that counts live blocks, records every size it is asked for and fails on request.
// Four slots hold a Buf each (or nothing).  One request per line on stdin:
//   new i        slot i: a new, empty Buf
//   delete i     slot i: destroyed (the destructor)
//   grow i n     slot i: grow(n); the block is then written from end to end
//   fail k       the next k allocations fail (error 7)
//   reset i      slot i: reset()
//   adopt i n    slot i: adopt(p, n) of a block of n bytes taken from the allocator here
//   movec i j    slot j: a new Buf move-constructed from slot i's
//   movea i j    slot j's Buf move-assigned from slot i's
// and one answer line each: grow's return value (0 for the other requests), every slot as "-" (nothing), "0:0" (empty) or "1:<bytes>"
// (a block, which is one the allocator has live), then what the allocator saw since the last line: the sizes asked for ("-": none),
// the number of frees, and the blocks live now.  At the end of input every slot is destroyed; the exit code is 0 only if no block is
// live then (3 if one is, 2 for a malformed request; a free of a block that is not live aborts).
// Built by tests/test_devbuf.py with the host compiler alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <utility>

#include "vhp_devbuf.hpp"

namespace {
struct Counting {
  static constexpr int ok = 0;
  static inline std::set<void*> live;
  static inline std::string asked;
  static inline int frees = 0, failing = 0;
  static int alloc(void** p, size_t bytes) {
    asked += (asked.empty() ? "" : ",") + std::to_string(bytes);
    if (failing > 0) { --failing; return 7; }
    *p = std::malloc(bytes);
    live.insert(*p);
    return ok;
  }
  static void free(void* p) {
    if (live.erase(p) != 1) std::abort();
    std::free(p);
    ++frees;
  }
};
using B = vhp::Buf<unsigned char, Counting>;
}  // namespace

int main() {
  std::unique_ptr<B> s[4];
  char what[16];
  int i;
  while (std::scanf("%15s %d", what, &i) == 2) {
    int rc = 0;
    size_t n = 0;
    int j = 0;
    const bool slot = std::strcmp(what, "fail") != 0;
    if (slot && (i < 0 || i > 3)) return 2;
    if (slot && std::strcmp(what, "new") != 0 && !s[i]) return 2;
    if (!std::strcmp(what, "new")) {
      s[i] = std::make_unique<B>();
    } else if (!std::strcmp(what, "delete")) {
      s[i].reset();
    } else if (!std::strcmp(what, "grow")) {
      if (std::scanf("%zu", &n) != 1) return 2;
      rc = s[i]->grow(n);
      if (s[i]->get()) std::memset(s[i]->get(), 0xAB, s[i]->bytes());
    } else if (!std::strcmp(what, "fail")) {
      Counting::failing = i;
    } else if (!std::strcmp(what, "reset")) {
      s[i]->reset();
    } else if (!std::strcmp(what, "adopt")) {
      if (std::scanf("%zu", &n) != 1) return 2;
      void* p = nullptr;
      if (Counting::alloc(&p, n) != Counting::ok) return 2;
      s[i]->adopt(static_cast<unsigned char*>(p), n);
    } else if (!std::strcmp(what, "movec")) {
      if (std::scanf("%d", &j) != 1 || j < 0 || j > 3 || j == i) return 2;
      s[j] = std::make_unique<B>(std::move(*s[i]));
    } else if (!std::strcmp(what, "movea")) {
      if (std::scanf("%d", &j) != 1 || j < 0 || j > 3 || j == i || !s[j]) return 2;
      *s[j] = std::move(*s[i]);
    } else {
      return 2;
    }
    std::printf("%d", rc);
    for (const auto& b : s) {
      if (!b) { std::printf(" -"); continue; }
      if ((b->get() != nullptr) != (b->bytes() != 0) || (b->get() && !Counting::live.count(b->get()))) return 4;
      std::printf(" %d:%zu", b->get() ? 1 : 0, b->bytes());
    }
    std::printf(" %s %d %zu\n", Counting::asked.empty() ? "-" : Counting::asked.c_str(), Counting::frees, Counting::live.size());
    Counting::asked.clear();
    Counting::frees = 0;
  }
  for (auto& b : s) b.reset();
  return Counting::live.empty() ? 0 : 3;
}
