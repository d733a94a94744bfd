// polar_own.hpp -- the owners of what the library takes from the HIP runtime: device memory (DBuf), pinned host memory
// (PinBuf), events and streams.  Each frees what it holds in its destructor, none can be copied, a moved-from one is empty: a
// handle made of them (polar_handle, polar_dist) needs no list of what to free, and one whose creation failed half-way leaves
// nothing behind.  With them the library's error types and the one place that turns an exception into a POLAR_ERR_* code
// (error_code).  Runtime API, standard library and the host-only pair_host.hpp -- no kernels, no handle --, so that a host
// compiler builds it against a stand-in runtime (tests/own).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "pair_host.hpp"

struct HipError : std::runtime_error {
  explicit HipError(const std::string &m) : std::runtime_error(m) {}
};
struct NoDevice : std::runtime_error {
  NoDevice() : std::runtime_error("no usable HIP device: this library has no CPU fallback") {}
};
// The exception in flight as the code an entry point returns, its text into `msg`: called inside a `catch (...)` (guarded,
// dist_guarded, the begin-agreement of polar_dist_step).  Anything that is no std::exception travels on.
inline int error_code(std::string &msg) {
  try {
    throw;
  } catch (const polar::InputError &e) { msg = e.what(); return POLAR_ERR_INPUT;
  } catch (const polar::Unsupported &e) { msg = e.what(); return POLAR_ERR_UNSUPPORTED;
  } catch (const NoDevice &e) { msg = e.what(); return POLAR_ERR_NO_DEVICE;
  } catch (const HipError &e) { msg = e.what(); return POLAR_ERR_HIP;
  } catch (const std::exception &e) { msg = e.what(); return POLAR_ERR_STATE; }
}
#define HIPCHECK(expr)                                                                             \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      throw HipError(std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" + __FILE__ + \
                     ":" + std::to_string(__LINE__) + ")");                                      \
  } while (0)

// device memory, grown with headroom and never shrunk; the contents do not survive a growth
template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(const DBuf &) = delete; DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DBuf &operator=(DBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~DBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    release();   // (empty from here until the new block is in hand: an allocation that throws leaves nothing dangling)
    size_t want = n + n / 8 + 64;
    T *q = nullptr;
    HIPCHECK(hipMalloc((void **)&q, want * sizeof(T)));
    p = q; cap = want;
    // POLAR_POISON=1 (debugging aid): a fresh process gets zero pages from hipMalloc, a long-lived one gets recycled memory --
    // fill every new buffer with 0x7F bytes (ints 2139062143, doubles 1.4e306) so that a read-before-write shows in the FIRST
    // call of a process instead of the ninetieth (the abort of round 4)
    static const bool poison = getenv("POLAR_POISON") && atoi(getenv("POLAR_POISON")) != 0;
    if (poison) {   // (the fill runs on the null stream, which the library's non-blocking streams do not wait for: finish it here)
      HIPCHECK(hipMemset(p, 0x7F, want * sizeof(T)));
      HIPCHECK(hipDeviceSynchronize());
    }
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// pinned host memory of exactly the size asked for (a caller that wants headroom asks for it: staging() in polar_handle.hpp)
template <typename T>
struct PinBuf {
  T *p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf &) = delete; PinBuf &operator=(const PinBuf &) = delete;
  PinBuf(PinBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  PinBuf &operator=(PinBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~PinBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    release();
    T *q = nullptr;
    HIPCHECK(hipHostMalloc((void **)&q, n * sizeof(T)));
    p = q; cap = n;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// one event; reads as the hipEvent_t it holds wherever one is recorded, waited for or timed
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete; Event &operator=(const Event &) = delete;
  Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
  Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = o.e; o.e = nullptr; } return *this; }
  ~Event() { release(); }
  void create() { release(); HIPCHECK(hipEventCreate(&e)); }
  void create(unsigned flags) { release(); HIPCHECK(hipEventCreateWithFlags(&e, flags)); }
  void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  operator hipEvent_t() const { return e; }
};

// one stream; reads as the hipStream_t it holds.  borrow(): a stream the caller owns stands in (polar_set_stream) and is
// never destroyed here.
struct Stream {
  hipStream_t s = nullptr;
  bool own_stream = true;
  Stream() = default;
  Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
  Stream(Stream &&o) noexcept : s(o.s), own_stream(o.own_stream) { o.s = nullptr; o.own_stream = true; }
  Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = o.s; own_stream = o.own_stream; o.s = nullptr; o.own_stream = true; } return *this; }
  ~Stream() { release(); }
  void create() { release(); HIPCHECK(hipStreamCreate(&s)); }
  void create(unsigned flags) { release(); HIPCHECK(hipStreamCreateWithFlags(&s, flags)); }
  void create(unsigned flags, int priority) { release(); HIPCHECK(hipStreamCreateWithPriority(&s, flags, priority)); }
  void borrow(hipStream_t foreign) { release(); s = foreign; own_stream = false; }
  void release() { if (s && own_stream) (void)hipStreamDestroy(s); s = nullptr; own_stream = true; }
  operator hipStream_t() const { return s; }
};
