// owned.h — move-only holders of the HIP resources csrc/ takes: each gives its resource back in its destructor, and nothing else in
// csrc/ calls the raw allocation / creation APIs (tests/test_abi.py holds that).  The holders keep a process-wide tally of what is
// live (urt_debug_live_resources).  Private.  A holder is reset with the device of its resource current, as it was made.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <utility>

#include "../../include/urt.h"

struct urt_context;

namespace urtd {

int fail(urt_context* ctx, int code, const std::string& msg);   // context.cpp: sets urt_last_error(ctx) (ctx NULL: the creation error); returns code

struct LiveResources { std::atomic<uint64_t> device_bytes{0}, pinned_bytes{0}, events{0}, streams{0}; };
inline LiveResources g_live;

// A handle H, what it weighs in its tally kLive (bytes; 1 per event or stream), and kDrop to give it back.
template <typename H, auto kDrop, auto kLive>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept { *this = std::move(o); }
  Owned& operator=(Owned&& o) noexcept { std::swap(h_, o.h_); std::swap(weight_, o.weight_); o.reset(); return *this; }
  ~Owned() { reset(); }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  void reset() {
    if (h_) { kDrop(h_); g_live.*kLive -= weight_; }
    h_ = nullptr; weight_ = 0;
  }

 protected:
  // takes over what a creation call made; a failed call leaves the holder empty, and its error is cleared and returned
  hipError_t adopt(hipError_t e, H h, uint64_t weight) {
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    h_ = h; weight_ = weight; g_live.*kLive += weight;
    return hipSuccess;
  }

 private:
  H h_ = nullptr;
  uint64_t weight_ = 0;
};
inline void free_device(void* p) { (void)hipFree(p); }
inline void free_pinned(void* p) { (void)hipHostFree(p); }
inline void destroy_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void destroy_stream(hipStream_t s) { (void)hipStreamDestroy(s); }

// cap() elements of T in device (kPinned: pinned host) memory.  alloc frees what is held, then allocates max(n * sizeof(T), min_bytes, 1)
// bytes (pinned: with hipHostMalloc's `flags`).
template <typename T, bool kPinned>
class OwnedBuf : public Owned<T*, kPinned ? free_pinned : free_device, kPinned ? &LiveResources::pinned_bytes : &LiveResources::device_bytes> {
 public:
  size_t cap() const { return *this ? n_ : 0; }
  hipError_t alloc(size_t n, size_t min_bytes = 0, unsigned int flags = hipHostMallocDefault) {
    this->reset();
    const size_t bytes = std::max<size_t>({n * sizeof(T), min_bytes, 1});
    void* p = nullptr;
    n_ = n;
    return this->adopt(kPinned ? hipHostMalloc(&p, bytes, flags) : hipMalloc(&p, bytes), (T*)p, bytes);
  }

 private:
  size_t n_ = 0;
};
template <typename T> using DeviceBuf = OwnedBuf<T, false>;
template <typename T> using PinnedBuf = OwnedBuf<T, true>;

struct Event : Owned<hipEvent_t, destroy_event, &LiveResources::events> {                // create(flags) replaces what is held
  hipError_t create(unsigned int flags) { reset(); hipEvent_t e = nullptr; return adopt(hipEventCreateWithFlags(&e, flags), e, 1); }
};
struct Stream : Owned<hipStream_t, destroy_stream, &LiveResources::streams> {
  hipError_t create(unsigned int flags) { reset(); hipStream_t s = nullptr; return adopt(hipStreamCreateWithFlags(&s, flags), s, 1); }
};

// THE grow-only policy of every device scratch: nothing to do while n elements fit; else work queued on `wait_for` (if any) may still
// use the old allocation and is waited for, then the buffer is replaced — its contents are not kept.  On failure the buffer is empty
// and the error names `what`.  A site with two scratches reserves both before it uses either.
template <typename T>
int reserve(urt_context* ctx, DeviceBuf<T>& buf, size_t n, const char* what, hipStream_t wait_for) {
  if (n <= buf.cap()) return URT_OK;
  hipError_t e = buf && wait_for ? hipStreamSynchronize(wait_for) : hipSuccess;
  if (e == hipSuccess) e = buf.alloc(n);
  if (e == hipSuccess) return URT_OK;
  return fail(ctx, e == hipErrorOutOfMemory ? URT_ERR_OUT_OF_MEMORY : URT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace urtd
