// scn_resource.h -- what the C-ABI layer owns on the device, as move-only members that release themselves.  Nothing is allocated
// in a constructor (every resource is created where it is first needed, under its own check); a pointer that only borrows stays
// raw.  Members go in reverse order of declaration: a struct declares its streams BEFORE the memory and events used on them, and
// whoever deletes it sets the device and synchronises the streams first.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// `count` elements of T in device memory (hipFree) or pinned host memory (hipHostFree)
template <class T, bool Pinned>
class ScnMemory {
 public:
  ScnMemory() = default;
  ScnMemory(ScnMemory &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  ScnMemory &operator=(ScnMemory &&o) noexcept {  // (o leaves with what this held, and releases it)
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~ScnMemory() { reset(); }
  T *get() const { return p_; }
  size_t capacity() const { return cap_; }  // elements allocated
  explicit operator bool() const { return p_ != nullptr; }
  hipError_t alloc(size_t count) {  // nothing when already allocated
    if (p_) return hipSuccess;
    const hipError_t e = Pinned ? hipHostMalloc(&p_, sizeof(T) * count, hipHostMallocDefault) : hipMalloc(&p_, sizeof(T) * count);
    if (e == hipSuccess) cap_ = count;
    else p_ = nullptr;
    return e;
  }
  hipError_t grow(size_t count) {  // a buffer grown on demand: frees first, and stays empty (capacity 0) when the allocation fails
    reset();
    return alloc(count);
  }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    cap_ = 0;
  }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};
template <class T>
using ScnDeviceMem = ScnMemory<T, false>;
template <class T>
using ScnPinnedMem = ScnMemory<T, true>;

template <class H, hipError_t (*Destroy)(H)>
class ScnHandle {
 public:
  ScnHandle() = default;
  ScnHandle(ScnHandle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  ScnHandle &operator=(ScnHandle &&o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  ~ScnHandle() {
    if (h_) (void)Destroy(h_);
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }

 protected:
  H h_ = nullptr;
};

struct ScnEvent : ScnHandle<hipEvent_t, hipEventDestroy> {  // (create: nothing when it exists, as alloc)
  hipError_t create(unsigned flags = hipEventDisableTiming) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
};
struct ScnStream : ScnHandle<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
  hipError_t create_with_priority(int priority) { return h_ ? hipSuccess : hipStreamCreateWithPriority(&h_, hipStreamNonBlocking, priority); }
  void sync() const {  // (teardown: a stream never created has nothing queued)
    if (h_) (void)hipStreamSynchronize(h_);
  }
};
