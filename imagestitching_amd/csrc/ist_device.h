// ist_device.h — the owners of everything the library asks the HIP runtime for: a device block, a pinned host block, a stream, an
// event.  Each is move-only, empty until its first grow() / ensure(), and gives its handle back in its destructor; the process-wide
// counts behind ist_debug_live_handles move where a handle is made and where it is released, nowhere else.
// No owner may live in static or thread-local storage: a destructor that runs after the HIP runtime has shut down is what the hosts'
// drain-at-exit hooks exist to avoid.  (The process-wide pinned result pool of ist_host.cpp is not built from these for that reason.)
#ifndef IST_DEVICE_H_
#define IST_DEVICE_H_

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <string>
#include <utility>

#include "ist_internal.h"

namespace ist {

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

enum LiveKind { kLiveDevice = 0, kLivePinned = 1, kLiveStream = 2, kLiveEvent = 3 };
extern std::atomic<int64_t> g_live_handles[4];      // (ist_runtime.cpp)
inline void live_count(LiveKind k, int64_t d) { g_live_handles[k].fetch_add(d, std::memory_order_relaxed); }

// a grow-only device block (dev_malloc: counted by ist_debug_device_allocs).  Freed with its own device current.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int device = -1;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(device, o.device); return *this; }
  ~DevBuf() { reset(); }
  // at least `need` bytes: nothing when the block is large enough, otherwise the block is freed FIRST and need + spare are allocated
  int grow(size_t need, size_t spare = 0) {
    if (bytes >= need) return IST_OK;
    reset();
    if (hipGetDevice(&device) != hipSuccess || dev_malloc(&p, need + spare) != 0) {
      (void)hipGetLastError(); p = nullptr;
      return fail(IST_E_NOMEM, "out of device memory (" + std::to_string((need + spare) >> 20) + " MiB)");
    }
    bytes = need + spare;
    live_count(kLiveDevice, 1);
    return IST_OK;
  }
  void reset() {
    if (!p) return;
    int cur = device;
    (void)hipGetDevice(&cur);
    if (cur != device) { DeviceGuard g(device); (void)hipFree(p); } else (void)hipFree(p);
    p = nullptr; bytes = 0;
    live_count(kLiveDevice, -1);
  }
};

// the same over hipHostMalloc (hipHostMallocDefault: memory only this library's copies read and write)
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
  ~PinnedBuf() { reset(); }
  int grow(size_t need, size_t spare = 0) {
    if (bytes >= need) return IST_OK;
    reset();
    if (hipHostMalloc(&p, need + spare, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(IST_E_NOMEM, "out of pinned host memory"); }
    bytes = need + spare;
    live_count(kLivePinned, 1);
    return IST_OK;
  }
  void reset() {
    if (!p) return;
    (void)hipHostFree(p);
    p = nullptr; bytes = 0;
    live_count(kLivePinned, -1);
  }
};

// a non-blocking stream, made on first use; waited for before it is destroyed
struct Stream {
  enum Priority { kDefault, kHighest, kLowest };
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
  ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); live_count(kLiveStream, -1); } }
  operator hipStream_t() const { return s; }
  int ensure(Priority pr = kDefault) {
    if (s) return IST_OK;
    int lo = 0, hi = 0;
    if (pr != kDefault) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    const hipError_t e = pr == kDefault ? hipStreamCreateWithFlags(&s, hipStreamNonBlocking) : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, pr == kLowest ? lo : hi);
    if (e != hipSuccess) { (void)hipGetLastError(); s = nullptr; return fail(IST_E_HIP, "hipStreamCreate failed"); }
    live_count(kLiveStream, 1);
    return IST_OK;
  }
};

// an event without timing, made on first use.  (An empty one destroys nothing: hipEventDestroy(NULL) would leave a sticky error for the
// next launch check.)
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { if (e) { (void)hipEventDestroy(e); live_count(kLiveEvent, -1); } }
  operator hipEvent_t() const { return e; }
  int ensure() {
    if (e) return IST_OK;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e = nullptr; return fail(IST_E_HIP, "hipEventCreate failed"); }
    live_count(kLiveEvent, 1);
    return IST_OK;
  }
};

}  // namespace ist

#endif  // IST_DEVICE_H_
