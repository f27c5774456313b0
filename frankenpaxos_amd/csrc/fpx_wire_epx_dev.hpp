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
#include "fpx_epx_cmd_parse.hpp"
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

// ---- the replica's inbox from wire bytes: fpx_wire_epx_classify_dev and fpx_wire_epx_replica_tick[_dev] ------------------
// What EPaxosNative.scala's classify and keyOf do on the JVM: the key list of every message's command
// (fpx_epx_cmd_parse.hpp, one thread per message, the parser the host classify of fpx_wire.cpp runs) as the CSR arrays the
// _mk calls take, the key strings interned in the context's key table (fpx_intern.hpp).
//   k_cls_count   shape, is_set, is_noop and the key count of every command
//   (k_epx_wire_replica_check, in a tick: kinds, dependency shapes and command shapes)
//   k_lr_bscan    (fpx_epx_leader.hpp) twice: the counts' exclusive scan inside rows of 1024 messages, then of the rows' sums
//   k_cls_decide  the pair count against max_pairs
//   (k_epx_wire_tail: the bad index, a bad tick becomes FPX_EINVAL)
//   k_cls_emit    key_offsets, and the parser again: (off, len) of every pair
//   the intern batch over the pairs, its ids written as `keys`
//   k_cls_result  the result block's new keys / new bytes
struct ClsBatch {
  const uint8_t* buf;
  int64_t buf_len;
  const int64_t* cmd_off;
  const int32_t* cmd_len;  // < 0: the message has no command (a Prepare): an empty list
  int32_t m, max_pairs;
  int32_t* key_offsets;    // [m + 1]
  uint8_t* is_set;
  int32_t *is_noop, *shape;
  int32_t* result;         // bad index, num_pairs, new keys, new bytes
  // scratch
  int32_t* cnt;            // [m]
  uint32_t* cscan;         // [m padded to rows of INTERN_ROW] the counts again, then their exclusive scan inside the row
  int32_t *ctot, *cgt;     // [rows] the rows' sums, then their exclusive scan; [1] the total
  int32_t* np;             // the pairs the intern batch runs over: 0 when the tick is refused
  int64_t* pair_off;       // [max_pairs]
  int32_t* pair_len;
};

// (the grid covers the messages padded to whole rows of the scan: the padding counts as zero)
__global__ void __launch_bounds__(256) k_cls_count(const EpxState st, const ClsBatch b) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  int32_t cnt = 0;
  if (i < b.m) {
    const int32_t len = b.cmd_len[i];
    fpxw::EpxCmd c;
    int32_t noop = -1, shape = -1;
    if (len >= 0) {
      const int64_t off = b.cmd_off[i];
      bool ok = off >= 0 && off <= b.buf_len - len;
      if (ok) {
        fpxw::EpxNoKeys none;
        ok = fpxw::epx_parse_command(fpxw::Reader{b.buf + off, b.buf + off + len}, &c, none);
      }
      if (!ok) epx_wire_bad(st, true, i);
      noop = c.is_noop, shape = c.shape;
    }
    cnt = c.num_keys;
    b.cnt[i] = cnt, b.is_set[i] = (uint8_t)c.is_set, b.is_noop[i] = noop, b.shape[i] = shape;
  }
  b.cscan[i] = (uint32_t)cnt;
}

// what fpx_wire_epx_replica_tick holds: PreAccept, Accept, Commit (of the context's n sets, in the burst calls' form, a
// canonical command) and Prepare; ri_kind = the kind codes of fpx_epx_replica_inbox
__global__ void __launch_bounds__(256) k_epx_wire_replica_check(const EpxState st, int32_t m, const int32_t* __restrict__ kind,
                                                                const int32_t* __restrict__ nr, const int32_t* __restrict__ shape,
                                                                const int32_t* __restrict__ cmd_shape, int32_t triple_base,
                                                                const int32_t* __restrict__ triple_in, int32_t* __restrict__ ri_kind,
                                                                int32_t* __restrict__ triple) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int32_t k = kind[i];
  int32_t rk = -1;
  if (k == FPX_WIRE_EPX_PREPARE) rk = FPX_EPX_IN_PREPARE;
  else if (nr[i] == st.n && shape[i] == 1 && cmd_shape[i] == 1)
    rk = k == FPX_WIRE_EPX_PRE_ACCEPT ? FPX_EPX_IN_PRE_ACCEPT
         : k == FPX_WIRE_EPX_ACCEPT   ? FPX_EPX_IN_ACCEPT
         : k == FPX_WIRE_EPX_COMMIT   ? FPX_EPX_IN_COMMIT
                                      : -1;
  if (rk < 0) epx_wire_bad(st, true, i);
  ri_kind[i] = rk < 0 ? 0 : rk;
  triple[i] = triple_in ? triple_in[i] : (rk == FPX_EPX_IN_PREPARE ? -1 : triple_base + i);
}

// one thread, behind the scans of the counts (k_lr_bscan, which stands back behind an FPX_EINVAL: the total is read only
// when the status is clean).  (A key is two bytes of a buffer < 2^31: the total fits.)
__global__ void k_cls_decide(const EpxState st, const ClsBatch b) {
  bool refused = st.status[0] != 0;  // (k_epx_wire_tail ran: a bad tick is the context's FPX_EINVAL by now)
  const int32_t total = refused ? 0 : *b.cgt;
  if (!refused && total > b.max_pairs) {
    epx_report(st.status, FPX_ECAPACITY, -1);
    refused = true;
  }
  b.result[1] = total;
  *b.np = refused ? 0 : total;
}

struct ClsPairSink {
  const uint8_t* base;
  int64_t* off;
  int32_t* len;
  int32_t first, cap;
  __device__ void key(int32_t j, const uint8_t* at, int32_t n) {
    const int64_t p = (int64_t)first + j;
    if (p < cap) off[p] = at - base, len[p] = n;
  }
};

__global__ void __launch_bounds__(256) k_cls_emit(const ClsBatch b) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.m) return;
  if (*b.np == 0 && b.result[1] == 0) {  // no pairs, or a call that was refused before they were counted
    b.key_offsets[i] = 0;
    if (i == b.m - 1) b.key_offsets[b.m] = 0;
    return;
  }
  const int32_t cnt = b.cnt[i];
  const int32_t first = (int32_t)(b.cscan[i] + (uint32_t)b.ctot[i / INTERN_ROW]);
  b.key_offsets[i] = first;
  if (i == b.m - 1) b.key_offsets[b.m] = first + cnt;
  if (cnt == 0 || *b.np == 0) return;
  const int64_t off = b.cmd_off[i];
  ClsPairSink s{b.buf, b.pair_off, b.pair_len, first, b.max_pairs};
  fpxw::EpxCmd c;
  (void)fpxw::epx_parse_command(fpxw::Reader{b.buf + off, b.buf + off + b.cmd_len[i]}, &c, s);
}

__global__ void k_cls_result(const ClsBatch b, const long long* ctl) {
  const long long bytes = ctl[IC_NEW_BYTES];
  b.result[2] = (int32_t)ctl[IC_NEW];
  b.result[3] = bytes > 0x7fffffff ? 0x7fffffff : (int32_t)bytes;
}
