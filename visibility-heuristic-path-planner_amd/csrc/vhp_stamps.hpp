// vhp_stamps.hpp -- the bookkeeping of the timestamps a pool-sweep or latency-sweep launch writes from inside its own kernels
// (vhp_pool.hip, vhp_lat.hip) in place of event records around it.  Host code without a HIP header: tests/stamps_driver.cpp runs it
// on the CPU.
//
// A stamp is one 16-byte entry {ticks, tag}: the device's constant-rate wall clock and the launch's epoch (vhp_ctx::pool_epoch, unique
// per launch on a context).  A launch owns one slot of entries: its begin entries first -- one, written by thread 0 of the launch's
// one-workgroup pre-kernel, or one per workgroup of a launch without a pre-kernel --, then one end entry per workgroup of the sweep
// kernel.  Nothing resets a slot and nothing counts: the clock is monotone, so the launch ran from the smallest begin entry to the
// largest end entry, and an entry that still carries another launch's tag says that this launch has not finished (or never ran): its
// time cannot be read.
//
// The slots are one array on the device: slot 0 for the launches of a context with vhp_timing off (each overwrites the one before: it
// serves vhp_last_elapsed_ms alone), slots 1 .. n a ring for the timed ones, handed out in order and given back oldest first by
// vhp_timing_collect.  A timed launch that finds the ring full, or that has more workgroups than a slot has entries for, is timed by an
// event pair as before.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vhp {
namespace stamps {

struct Entry {
  unsigned long long ticks, tag;
};
static_assert(sizeof(Entry) == 16, "one 16-byte store per stamp");

// A slot holds a launch of up to `groups` workgroups whether or not it has a pre-kernel: `groups` begin entries and `groups` end entries.
constexpr size_t slot_entries(int groups) { return groups > 0 ? 2 * (size_t)groups : 0; }
constexpr size_t slot_bytes(int groups) { return slot_entries(groups) * sizeof(Entry); }

// The ring of vhp_timing (slots 1 .. n; slot 0 is the untimed launches').
class Ring {
 public:
  // n slots for launches of up to `groups` workgroups: only while no slot is out (else nothing changes, and false)
  bool resize(int n, int groups) {
    if (live_ != 0) return n_ == n && groups_ == groups;
    n_ = n > 0 ? n : 0;
    groups_ = groups > 0 ? groups : 0;
    head_ = 0;
    return true;
  }
  int slots() const { return n_; }
  int groups() const { return groups_; }
  int live() const { return live_; }
  size_t bytes() const { return (size_t)(n_ + 1) * slot_bytes(groups_); }   // (with slot 0)
  size_t slot_offset(int slot) const { return (size_t)slot * slot_entries(groups_); }   // in entries
  bool fits(int n_begin, int n_end) const { return n_begin >= 1 && n_end >= 1 && (size_t)n_begin + (size_t)n_end <= slot_entries(groups_); }

  // the next slot (1 .. n), or -1: every slot is out -- the caller falls back to events, it is never handed a slot that is still unread
  int take() {
    if (live_ >= n_) return -1;
    const int slot = 1 + head_;
    head_ = (head_ + 1) % n_;
    ++live_;
    return slot;
  }
  // the newest slot back, for a launch that did not go out
  void untake() {
    if (live_ == 0) return;
    head_ = (head_ + n_ - 1) % n_;
    --live_;
  }
  int oldest() const { return live_ ? 1 + (head_ + n_ - live_) % n_ : -1; }
  // the k oldest slots back (vhp_timing_collect has read them)
  void release(int k) { live_ -= k < live_ ? k : live_; }
  // The slots that are out, oldest first, as at most two runs of neighbours [first, first + count): what to copy from the device.
  int runs(int first[2], int count[2]) const {
    if (live_ == 0) return 0;
    const int o = oldest();
    const int to_end = n_ - (o - 1);
    first[0] = o;
    count[0] = live_ < to_end ? live_ : to_end;
    if (count[0] == live_) return 1;
    first[1] = 1;
    count[1] = live_ - count[0];
    return 2;
  }

 private:
  int n_ = 0, groups_ = 0, head_ = 0, live_ = 0;
};

// What a stamped launch keeps on the host: its slot, how many entries of each kind it writes, its tag and the stream it went out on.
struct Launch {
  int slot = -1;   // -1: not stamped
  int n_begin = 0, n_end = 0;
  unsigned long long tag = 0;
  void* stream = nullptr;
  bool stamped() const { return slot >= 0; }
};

// ticks of a clock of `khz` kHz (hipDeviceAttributeWallClockRate) in milliseconds
inline float ticks_to_ms(unsigned long long ticks, int khz) { return khz > 0 ? (float)((double)ticks / (double)khz) : 0.0f; }

struct Time {
  bool ok = false;
  float ms = 0.0f;
};

// A slot's host copy to the launch's time: every expected entry must carry the launch's tag, and the last end not lie before the
// first begin.
inline Time reduce(const Entry* slot, const Launch& l, int khz) {
  Time t;
  if (!slot || !l.stamped() || l.n_begin < 1 || l.n_end < 1 || khz <= 0) return t;
  unsigned long long b = ~0ull, e = 0;
  for (int k = 0; k < l.n_begin; ++k) {
    if (slot[k].tag != l.tag) return t;
    if (slot[k].ticks < b) b = slot[k].ticks;
  }
  for (int k = 0; k < l.n_end; ++k) {
    const Entry& s = slot[l.n_begin + k];
    if (s.tag != l.tag) return t;
    if (s.ticks > e) e = s.ticks;
  }
  if (e < b) return t;
  t.ok = true;
  t.ms = ticks_to_ms(e - b, khz);
  return t;
}

// What vhp_last_elapsed_ms reports: nothing, the context's event pair, a stamped launch that is still to be read, or a time that has
// been read (a launch whose slot vhp_timing_collect gave back, or one read before).  A launch that fails leaves this as it was.
struct Last {
  enum State { kNothing, kEvents, kStamps, kRead };
  State state = kNothing;
  Launch launch;     // kStamps, kRead
  Time time;         // kRead
  void nothing() { state = kNothing; }
  void events() { state = kEvents; }
  void stamps(const Launch& l) { state = kStamps; launch = l; }
  // a reader (vhp_timing_collect, vhp_last_elapsed_ms) has reduced launch `tag`: kept if that is the launch this stands for, so that
  // both calls report one number and the slot may go back to the ring
  void read(unsigned long long tag, const Time& t) {
    if (state == kStamps && launch.tag == tag) { state = kRead; time = t; }
  }
};

}  // namespace stamps
}  // namespace vhp
