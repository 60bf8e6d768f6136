// One statement of a device workspace's layout, for its size and for its pointers.  A stage writes one layout function
// that takes its dimensions and a Carver& and `take`s its arrays in order.  Run on a measuring carver
// (default-constructed, no memory behind it) it yields the byte count the entry point allocates; run on a carving
// carver (over the allocated buffer) it yields the device pointers, and fits() tells whether the buffer holds them.
// A launch function returns -5 before its first launch when it does not.  A sub-stage's workspace is the sub-stage's
// layout function called on the same carver.
// Host-only: no HIP include, so tests/workspace_check.cpp runs it without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mq {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

class Carver {
 public:
  Carver() = default;
  // base must be 256-byte aligned (hipMalloc's alignment): every take's alignment is relative to it
  Carver(void* base, size_t bytes) : base_(reinterpret_cast<uintptr_t>(base)), bytes_(bytes), carving_(true) {
    if (base_ & 255) failed_ = true;
  }

  // aligns the offset up to `align` (a power of two, at least alignof(T)), then reserves count * sizeof(T) bytes.
  // A measuring carver returns the offset as a pointer; nobody dereferences it.
  template <class T>
  T* take(size_t count, size_t align = 256) {
    if ((align & (align - 1)) || align < alignof(T)) failed_ = true;
    const size_t at = (at_ + align - 1) & ~(align - 1);
    if (failed_ || at < at_ || count > (SIZE_MAX - at) / sizeof(T)) {
      failed_ = true;
      return nullptr;
    }
    at_ = at + count * sizeof(T);
    return reinterpret_cast<T*>(base_ + at);
  }

  size_t used() const { return failed_ ? SIZE_MAX : at_; }
  bool fits() const { return carving_ && !failed_ && at_ <= bytes_; }

 private:
  uintptr_t base_ = 0;
  size_t bytes_ = 0, at_ = 0;
  bool carving_ = false, failed_ = false;
};

// the byte count of a layout: `layout(carver, dims...)` run on a measuring carver
template <class F, class... A>
size_t measure(F layout, A... dims) {
  Carver c;
  layout(c, dims...);
  return c.used();
}

}  // namespace mq
