// TEST INFRASTRUCTURE -- a stand-in for the handful of HIP runtime calls the owners of csrc/polar_own.hpp use, over malloc,
// so that tests/own/own_host.cpp runs them on the host under the address sanitizer: a block freed twice, used after its
// release or never freed is the sanitizer's finding, and the counts of live objects per kind say the same from the inside.
// fake_fail_nth(n): the n-th allocation from now on (device or pinned memory) fails with hipErrorOutOfMemory.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

namespace {
enum { MEM = 0, PIN, EVENT, STREAM, KINDS };
long g_live[KINDS] = {0, 0, 0, 0};
long g_allocs = 0;       // successful memory allocations so far
long g_fail_in = 0;      // > 0: that many allocations from now, one fails

hipError_t take(void **out, size_t bytes, int kind) {
  if (kind == MEM || kind == PIN) {
    if (g_fail_in > 0 && --g_fail_in == 0) return hipErrorOutOfMemory;   // (*out is left alone, as a real failure may)
    g_allocs++;
  }
  *out = malloc(bytes ? bytes : 1);
  if (!*out) return hipErrorOutOfMemory;
  g_live[kind]++;
  return hipSuccess;
}
hipError_t give(void *p, int kind) {
  if (!p) return hipSuccess;
  free(p);
  g_live[kind]--;
  return hipSuccess;
}
}  // namespace

extern "C" {
long fake_live(int kind) { return g_live[kind]; }
long fake_allocs(void) { return g_allocs; }
void fake_fail_nth(long n) { g_fail_in = n; }

hipError_t hipMalloc(void **ptr, size_t size) { return take(ptr, size, MEM); }
hipError_t hipFree(void *ptr) { return give(ptr, MEM); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return take(ptr, size, PIN); }
hipError_t hipHostFree(void *ptr) { return give(ptr, PIN); }
hipError_t hipEventCreate(hipEvent_t *e) { return take((void **)e, 1, EVENT); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return take((void **)e, 1, EVENT); }
hipError_t hipEventDestroy(hipEvent_t e) { return give((void *)e, EVENT); }
hipError_t hipStreamCreate(hipStream_t *s) { return take((void **)s, 1, STREAM); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return take((void **)s, 1, STREAM); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { return take((void **)s, 1, STREAM); }
hipError_t hipStreamDestroy(hipStream_t s) { return give((void *)s, STREAM); }
hipError_t hipMemset(void *dst, int value, size_t bytes) { memset(dst, value, bytes); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (fake)" : "error (fake)"; }
}
