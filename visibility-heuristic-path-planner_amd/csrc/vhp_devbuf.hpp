// vhp_devbuf.hpp -- the one owner of a piece of device or pinned memory: every grow-only scratch and every state array of the host
// code is a Buf.  A pointer and its size in bytes, move-only, freed when it goes.  Host code without a HIP header: the memory comes
// from Alloc (vhp_devbuf.hip.h: hipMalloc, hipHostMalloc), and tests/devbuf_driver.cpp puts an allocator that counts and fails in its
// place, on the CPU.
//   Alloc::ok                  what alloc returns when it has allocated
//   Alloc::alloc(void**, n)    n > 0 bytes, or an error code
//   Alloc::free(void*)
#pragma once
#include <cstddef>

namespace vhp {

template <class T, class Alloc>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; bytes_ = o.bytes_;
      o.p_ = nullptr; o.bytes_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  T* get() const { return p_; }
  size_t bytes() const { return bytes_; }

  // Room for `bytes`: nothing happens while the buffer holds that much (and for bytes == 0); else it is freed and allocated anew,
  // contents not kept.  A failed allocation leaves the buffer empty -- never a null pointer beside the old size -- and returns
  // Alloc's error.
  auto grow(size_t bytes) -> decltype(Alloc::alloc(nullptr, bytes)) {
    if (bytes_ >= bytes) return Alloc::ok;
    reset();
    void* p = nullptr;
    const auto e = Alloc::alloc(&p, bytes);
    if (e != Alloc::ok) return e;
    p_ = static_cast<T*>(p);
    bytes_ = bytes;
    return e;
  }

  void reset() {
    if (p_) Alloc::free(p_);
    p_ = nullptr;
    bytes_ = 0;
  }

  // Takes over `bytes` at p, which the caller allocated and Alloc::free can free.
  void adopt(T* p, size_t bytes) {
    reset();
    p_ = p;
    bytes_ = bytes;
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace vhp
