// fpx_host.hpp -- the host plumbing that fpx_api.hip (fpx_ctx) and fpx_epaxos.hip (fpx_epx) share: device buffers that
// grow, carved scratch, and host_call, the driver of every host-pointer entry point (its arrays: fpx_host_call.hpp).
// Written against what the two contexts have in common: a `stream`, a `last_hip` word that keeps the HIP error of a failed
// call, and a HostStage `stage`.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "../../include/fpx.h"
#include "fpx_host_call.hpp"
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

// ---- host-pointer calls: stage, launch, copy back ------------------------------------------------------------------
// what a context keeps for them: the staging buffer every array of a call is carved from, and the host buffer of the held
// outputs (pageable, grows, never shrinks)
struct HostStage {
  DevBuf dev;
  char* held = nullptr;
  size_t held_cap = 0;
};
inline void free_stage(HostStage* s) {
  if (s->dev.p) (void)hipFree(s->dev.p);
  free(s->held);
  *s = HostStage();
}

// grows the staging buffer once to hold every array (and the host buffer of the held outputs: FPX_ENOMEM with nothing
// enqueued), points the slots at their arrays, uploads the inputs and enqueues the fills
template <typename Ctx>
int stage_arrays(Ctx* ctx, std::initializer_list<Staged> arrays, const StageLayout& l) {
  HostStage& s = ctx->stage;
  const int rc = grow(ctx, &s.dev, l.total);
  if (rc) return rc;
  if (l.held_total > s.held_cap) {
    char* h = static_cast<char*>(malloc(l.held_total));
    if (!h) return FPX_ENOMEM;
    free(s.held);
    s.held = h, s.held_cap = l.held_total;
  }
  char* const base = (char*)s.dev.p;
  size_t i = 0;
  for (const Staged& a : arrays) {
    char* const p = base + l.at[i++];
    a.place(a.slot, p);
    if (a.src && a.bytes) HIPCHK(ctx, hipMemcpyAsync(p, a.src, a.bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  for (const StageLayout::Fill& f : l.fills) HIPCHK(ctx, hipMemsetAsync(base + f.at, f.value, f.bytes, ctx->stream));
  return FPX_OK;
}

// enqueues the downloads: an output to the caller's array, a held one (whether the caller wants it or not: a count may
// be read) to the host buffer
template <typename Ctx>
int fetch_arrays(Ctx* ctx, std::initializer_list<Staged> arrays, const StageLayout& l) {
  const HostStage& s = ctx->stage;
  size_t i = 0;
  for (const Staged& a : arrays) {
    void* const to = a.hold ? s.held + l.held_at[i] : a.dst;
    if (to && a.bytes) HIPCHK(ctx, hipMemcpyAsync(to, (const char*)s.dev.p + l.at[i], a.bytes, hipMemcpyDeviceToHost, ctx->stream));
    ++i;
  }
  return FPX_OK;
}

// the held outputs, downloaded and the stream synchronised, go to the caller
inline void deliver_held(const HostStage& s, std::initializer_list<Staged> arrays, const StageLayout& l) {
  size_t i = 0;
  for (const Staged& a : arrays) {
    if (a.hold && a.dst) {
      const size_t len = l.length_at[i];
      const size_t bytes = len == StageLayout::NONE ? a.bytes : (size_t)*reinterpret_cast<const int32_t*>(s.held + len) * 4;
      memcpy(a.dst, s.held + l.held_at[i], bytes);
    }
    ++i;
  }
}

// The driver of the host-pointer entry points: lays the arrays out (lay_stage), stages them, runs launch(), checks the
// launches, enqueues the downloads, and ends the call the context's way: end() synchronises and returns the call's
// status, and end.applied(status) says whether that status lets the held outputs reach the caller.  The host checks of a
// call come before it: nothing is staged on a bad batch.
template <typename Ctx, typename Launch, typename End>
int host_call(Ctx* ctx, std::initializer_list<Staged> arrays, Launch launch, End end) {
  const StageLayout l = lay_stage(arrays);
  int rc;
  if ((rc = stage_arrays(ctx, arrays, l)) || (rc = launch()) || (rc = launch_check(ctx)) || (rc = fetch_arrays(ctx, arrays, l)))
    return rc;
  rc = end();
  if (end.applied(rc)) deliver_held(ctx->stage, arrays, l);
  return rc;
}

}  // namespace fpx
