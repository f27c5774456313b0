// fpx_wire_epx_dev.hpp -- EPaxos ReplicaInbound messages decoded on the device (include/fpx_wire.h,
// fpx_wire_epaxos_decode_replica_inbound_dev and fpx_wire_epx_leader_tick[_dev]).  Included by fpx_epaxos.hip inside its
// anonymous namespace.  One thread per message runs the parser of fpx_wire_epx_parse.hpp with its folded sink, the code
// the g++-compiled fpx_wire_epaxos_decode_replica_inbound_folded runs, so the two agree by construction
// (tests/test_gpu_epaxos_wire_dev.py compares them array for array all the same).
//
// A PreAcceptOk at n = 5 is about 50 bytes, nested four deep (member, dependencies, set, packed values); the thread reads
// it byte by byte, twice where it has dependencies (the second pass folds them against the instance, which may follow
// them in byte order).  A wavefront's 64 messages span ~3 KB that the first touch brings into the cache; HBM sees each
// byte once.  The watermark row is num_replicas 4-byte stores per thread at a stride of the row length.
//
// Errors: as k_wire_decode (fpx_wire_dev.hpp).  A word of the context's status block collects the first offender under
// atomicMax -- a bad offset outranks a malformed message, the lower index wins -- and one thread then turns it into the
// bad index and the context's FPX_EINVAL, behind which every later kernel of the stream stands back.
#pragma once
#include "fpx_wire_epx_parse.hpp"

enum { EPX_ST_WIRE = 2 };  // status word: 0x7fffffff - key of the first bad message, 0 = none

__device__ __forceinline__ void epx_wire_bad(const EpxState& st, bool parse, int32_t i) {
  atomicMax(&st.status[EPX_ST_WIRE], 0x7fffffff - ((parse ? 0x40000000 : 0) + i));
}

__global__ void __launch_bounds__(256) k_epx_wire_decode(const EpxState st, const uint8_t* __restrict__ buf, int64_t buf_len,
                                                         const int64_t* __restrict__ offsets, int32_t n, int32_t num_replicas,
                                                         const fpxw::EpxFoldOut o) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool bounds = fpxw::offset_ok(offsets, i, buf_len);
  if (!bounds) epx_wire_bad(st, false, i);
  if (!fpxw::offset_ok(offsets, i + 1, buf_len)) {
    if (i == n - 1) epx_wire_bad(st, false, i);  // the last offset has no message of its own to blame
    bounds = false;
  }
  // (out of bounds: an empty message, so that every array has its row all the same)
  const uint8_t* at = buf + (bounds ? offsets[i] : 0);
  fpxw::Reader r{at, bounds ? buf + offsets[i + 1] : at};
  if (!fpxw::epx_decode_folded(buf, r, i, num_replicas, o)) epx_wire_bad(st, true, i);
}

// what fpx_wire_epx_leader_tick holds: PreAcceptOk (of the context's n sets, in the burst calls' form), AcceptOk, Nack.
// Anything else is refused like a malformed message; lr_kind = the kind codes of fpx_epx_leader_replies.  A Nack has no
// replica_index on the wire (-1 from the decoder): it gets 0, which fpx_epx_leader_replies checks and never reads
__global__ void __launch_bounds__(256) k_epx_wire_tick_check(const EpxState st, int32_t m, const int32_t* __restrict__ kind,
                                                             const int32_t* __restrict__ nr, const int32_t* __restrict__ shape,
                                                             int32_t* __restrict__ lr_kind, int32_t* __restrict__ ridx) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int32_t k = kind[i];
  int32_t lr = -1;
  if (k == FPX_WIRE_EPX_PRE_ACCEPT_OK && nr[i] == st.n && shape[i] == 1) lr = LR_PRE_ACCEPT_OK;
  else if (k == FPX_WIRE_EPX_ACCEPT_OK) lr = LR_ACCEPT_OK;
  else if (k == FPX_WIRE_EPX_NACK) lr = LR_NACK, ridx[i] = 0;
  if (lr < 0) epx_wire_bad(st, true, i);
  lr_kind[i] = lr;
}

// one thread: the bad index (always written), and a bad tick becomes the context's FPX_EINVAL
__global__ void k_epx_wire_tail(const EpxState st, int32_t* bad_index) {
  const int32_t w = st.status[EPX_ST_WIRE];
  const int32_t bad = w == 0 ? -1 : ((0x7fffffff - w) & 0x3fffffff);
  if (bad_index) *bad_index = bad;
  if (w == 0) return;
  st.status[EPX_ST_WIRE] = 0;
  epx_report(st.status, FPX_EINVAL, bad);
}
