// fpx_host.hpp -- the host plumbing that fpx_api.hip (fpx_ctx) and fpx_epaxos.hip (fpx_epx) share.  Written against what
// the two contexts have in common: a `last_hip` word that keeps the HIP error of a failed call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "../../include/fpx.h"
#include "fpx_scratch.hpp"

namespace fpx {

// a device allocation that only grows
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
constexpr size_t DEVBUF_MIN_BYTES = 4096;  // the least grow() allocates, so a buffer of a few words is not freed and
                                           // allocated again for every somewhat larger call

// a failed HIP call leaves its error in the context (where there is one) and the entry point with FPX_ENOMEM / FPX_EHIP
#define HIPCHK(ctx, expr)                       \
  do {                                          \
    hipError_t _e = (expr);                     \
    if (_e != hipSuccess) {                     \
      if (ctx) (ctx)->last_hip = (int)_e;       \
      return _e == hipErrorOutOfMemory ? FPX_ENOMEM : FPX_EHIP; \
    }                                           \
  } while (0)

// The context's device is current inside an entry point and the caller's is restored on return: allocations (staging
// buffers, events) and launches otherwise land on whatever device the calling thread last selected -- two contexts on two
// GPUs in one process (or a torch.cuda.set_device elsewhere) would fault.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  DeviceScope() = default;
  explicit DeviceScope(int device) { enter(device); }
  void enter(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceScope() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// at least `bytes` in b; what it held is NOT kept
template <typename Ctx>
int grow(Ctx* ctx, DevBuf* b, size_t bytes) {
  if (bytes <= b->cap) return FPX_OK;
  if (b->p) HIPCHK(ctx, hipFree(b->p));
  b->p = nullptr;
  b->cap = 0;
  const size_t cap = std::max(bytes, DEVBUF_MIN_BYTES);
  HIPCHK(ctx, hipMalloc(&b->p, cap));
  b->cap = cap;
  return FPX_OK;
}

// after the launches of an entry point: a launch that failed (bad configuration, no such kernel) is reported here
template <typename Ctx>
int launch_check(Ctx* ctx) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ctx->last_hip = (int)e;
    return FPX_EHIP;
  }
  return FPX_OK;
}

// A call's scratch, cut into arrays by `lay` (fpx_scratch.hpp): the layout runs over a null base for the size the buffer
// must have, and again over the buffer
template <typename Ctx, typename S, typename Lay>
int carve(Ctx* ctx, DevBuf* buf, S* out, Lay lay) {
  Carver size(nullptr);
  (void)lay(size);
  const int rc = grow(ctx, buf, size.size());
  if (rc) return rc;
  Carver c(buf->p);
  *out = lay(c);
  return FPX_OK;
}

}  // namespace fpx
