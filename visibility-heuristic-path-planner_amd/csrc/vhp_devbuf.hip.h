// vhp_devbuf.hip.h -- the two kinds of memory the host code owns through vhp::Buf (vhp_devbuf.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "vhp_devbuf.hpp"

namespace vhp {

// (a free is a plain hipFree / hipHostFree: it waits for whatever still reads the memory)
struct HipDevice {
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct HipPinned {
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static void free(void* p) { (void)hipHostFree(p); }
};

template <class T> using DevBuf = Buf<T, HipDevice>;
template <class T> using PinnedBuf = Buf<T, HipPinned>;

}  // namespace vhp
