// Status plumbing shared by the C-ABI translation units (capi_*.hip, precompute.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/gpmdm_hip.h"

namespace gpmdm {

extern thread_local std::string g_err;   // gpmdm_last_error()
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return ::gpmdm::fail(GPMDM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define CHECK(cond, msg)                                                                   \
  do {                                                                                     \
    if (!(cond)) return ::gpmdm::fail(GPMDM_E_INVALID, msg);                               \
  } while (0)

#define TRY(expr)                                                                          \
  do {                                                                                     \
    int rc_ = (expr);                                                                      \
    if (rc_ != GPMDM_OK) return rc_;                                                       \
  } while (0)

// The library's memory (memory.hip): device buffers are stream-ordered pool allocations made
// and released on a per-device lifecycle stream -- releasing one never synchronises the device
// (hipFree does) -- and pinned host buffers come from a size-class cache (hipHostFree also
// synchronises the device).  dfree's precondition: no launch still reads the buffer (the
// handle has waited for its own work), or use dfree_after(p, s) to order the release after
// stream s's work.
hipStream_t life_stream(int device);
hipStream_t life_stream_current();
int dev_alloc(void** p, size_t bytes);
void dev_free(void* p);
void dev_free_after(void* p, hipStream_t after);
int host_alloc(void** p, size_t bytes, unsigned flags);
void host_free(void* p);

template <typename T>
int dalloc(T** p, size_t n) {
  if (n == 0) n = 1;
  void* q = nullptr;
  const int rc = dev_alloc(&q, n * sizeof(T));
  *p = static_cast<T*>(q);
  return rc;
}

template <typename T>
void dfree(T*& p) {
  dev_free((void*)p);
  p = nullptr;
}

template <typename T>
void dfree_after(T*& p, hipStream_t after) {
  dev_free_after((void*)p, after);
  p = nullptr;
}

template <typename T>
int halloc(T** p, size_t n, unsigned flags) {
  void* q = nullptr;
  const int rc = host_alloc(&q, (n ? n : 1) * sizeof(T), flags);
  *p = static_cast<T*>(q);
  return rc;
}

template <typename T>
void hfree(T*& p) {
  host_free((void*)p);
  p = nullptr;
}

// ---- Owning types: what a handle holds is released with it, in the order memory.hip gives ----
// A device buffer from the pool.  Converts to T*, so launch code reads as with a raw pointer.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;                      // elements
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {                     // dfree's precondition: no launch still reads it
    dfree(p);
    cap = 0;
  }
  void release_after(hipStream_t s) {  // ... or the release ordered after s's earlier work
    dfree_after(p, s);
    cap = 0;
  }
  int alloc(size_t n) {
    release();
    TRY(dalloc(&p, n));
    cap = n;
    return GPMDM_OK;
  }
  // at least n elements, contents not kept; inside a call on stream s
  int grow(size_t n, hipStream_t s) {
    if (p && cap >= n) return GPMDM_OK;
    release_after(s);
    return alloc(n);
  }
};

// A pinned host buffer; mapped (fine-grained) ones carry their device view.
template <typename T>
struct PinBuf {
  T* p = nullptr;
  T* dev = nullptr;                    // mapped: the kernels' view of p
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p(o.p), dev(o.dev) { o.p = o.dev = nullptr; }
  PinBuf& operator=(PinBuf&&) = delete;
  ~PinBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    hfree(p);
    dev = nullptr;
  }
  int alloc(size_t n) {
    release();
    return halloc(&p, n, 0);
  }
  int alloc_mapped(size_t n) {
    release();
    TRY(halloc(&p, n, hipHostMallocMapped | hipHostMallocCoherent));
    void* v = nullptr;
    HIPCHK(hipHostGetDevicePointer(&v, p, 0));
    dev = static_cast<T*>(v);
    return GPMDM_OK;
  }
};

// An ordering event (no timing), created by its first record.  One never recorded has
// nothing to wait for.
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t record(hipStream_t s) {
    if (!e) {
      const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
      if (rc != hipSuccess) return rc;
    }
    return hipEventRecord(e, s);
  }
  hipError_t sync() const { return e ? hipEventSynchronize(e) : hipSuccess; }             // the host waits
  hipError_t block(hipStream_t s) const { return e ? hipStreamWaitEvent(s, e, 0) : hipSuccess; }   // s waits
};

// Results that land in a pinned buffer (the pose read-out, forecast, smoothed read-out and
// innovation calls): the device result, its landing buffer, and the event behind the call's
// launches with its flag -- the handle's lifecycle waits (capi_pf.hip quiesce) go through wait().
struct Landing {
  DevBuf<double> dev;
  PinBuf<double> pin;
  Event ev;
  bool pending = false;
  int reserve(size_t n, hipStream_t s) {
    if (dev && dev.cap >= n) return GPMDM_OK;
    pin.release();
    TRY(dev.grow(n, s));
    return pin.alloc(n);
  }
  // after the call's launches and copy-back on s (rc: theirs): the event is recorded whether
  // or not they succeeded, so wait() covers a call that fails before its own wait
  int finish(int rc, hipStream_t s) {
    pending = ev.record(s) == hipSuccess;
    if (rc != GPMDM_OK) return rc;
    HIPCHK(hipStreamSynchronize(s));
    pending = false;
    return GPMDM_OK;
  }
  int leave_pending(hipStream_t s) {   // launched only: the lifecycle waits for it
    HIPCHK(ev.record(s));
    pending = true;
    return GPMDM_OK;
  }
  int wait() {
    if (pending) {
      HIPCHK(ev.sync());
      pending = false;
    }
    return GPMDM_OK;
  }
};

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

}  // namespace gpmdm
