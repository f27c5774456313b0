// fpx_wire_epx_enc_dev.hpp -- the replies of a replica tick encoded on the device (include/fpx_wire.h,
// fpx_wire_epx_encode_replica_replies_dev and fpx_wire_epx_replica_tick_bytes[_dev]).  Included by fpx_epaxos.hip inside its
// anonymous namespace.  The records fpx_epx_replica_inbox[_mk] leaves in HBM become the serialised ReplicaInbound messages
// the replicas send back, with one offset PER MESSAGE (reply i goes to the sender of message i: nothing is compacted away,
// a message without a reply is an empty span).  The bytes and the decision which record becomes which reply are
// fpx_wire_epx_emit.hpp's, the source the host batch encoder compiles, so the two agree by construction;
// tests/test_gpu_epaxos_reply_encode.py holds them equal all the same.
//
// A variable-length stream compaction, as fpx_wire_enc_dev.hpp:
//   k_ere_len    one thread per record: the reply's kind and its length from the closed-form *_len, written as the element of
//                the scan; per wavefront the two counts (encoded, deferred), one ballot each
//   k_lr_bscan   (fpx_epx_leader.hpp) twice, as the classify uses it: the lengths' exclusive scan inside rows of 1024 records,
//                then of the rows' sums.  The scan is 32 bits wide, so one call encodes less than 4 GiB of replies
//   k_ere_decide ONE workgroup: the bytes needed as a 64-bit sum of the rows' sums, the totals, the verdict
//   k_ere_emit   one thread per record again: its offset from the two levels of the scan, out_offsets, reply_kind, and the
//                bytes -- in one of two forms:
//     span    every lane emits into its own LDS slot of ERE_SLOT bytes; the wavefront then writes the span of its 64
//             replies as aligned 16-byte words (lane l assembles piece l, l + 64, ... from the slots, finding a byte's
//             record by one binary search over the wavefront's 65 offsets per piece) and single bytes only at the ragged ends
//     direct  every lane runs the Writer at its own offset of the output: byte stores to HBM.  A wavefront that holds a
//             reply longer than ERE_SLOT (a PreAcceptOk with explicit ids, or one with wide watermarks at n = 7) goes this
//             way whole; FPX_EPX_ENC_DIRECT in the environment of fpx_epx_create sends every wavefront this way (the A/B of
//             profiles/epx_wire_replica_replies.md).  So does a wavefront that holds a reply with a stored command (a Commit
//             back, a PrepareOk of a seen instance: fpx_wire_epx_encode_replica_replies_cmds_dev): the lane writes the
//             fields in front of and behind the command, and the command's bytes are copied from the store's arena by the
//             whole wavefront, one command after the other (cmds_wave_copy of fpx_epx_cmds.hpp, the store's own copy).
// wave64; plain C++ stores only.
//
// Errors are PER-CALL codes, kept in status words of their own (EPX_ST_ENC): a reply buffer that is too small
// (FPX_ECAPACITY) or an outcome outside 0 .. 8 (FPX_EINVAL) stops THIS encode; no later kernel of the context stands back
// behind it, and fpx_epx_sync returns and clears it like any status.
#pragma once
#include "fpx_epx_cmds.hpp"
#include "fpx_wire_epx_emit.hpp"

enum { EPX_ST_ENC = 3, EPX_ST_ENC_INDEX = 4 };  // status words: the encoder's per-call code and its index
constexpr int ERE_BLOCK = 256;                  // records per workgroup
constexpr int ERE_SLOT = 100;                   // LDS bytes per reply: 25 words, an odd stride over the banks
constexpr int32_t ERE_NO_BAD = 0x7f7f7f7f;      // (what a one-byte memset leaves: above any record index)
enum { ERE_C_BAD = 0, ERE_C_GO = 1, ERE_C_ENCODED = 2, ERE_C_DEFERRED = 3, ERE_C_WORDS = 4 };

struct EreArgs {
  fpxw::EpxReplyIn in;
  int32_t m, rows, direct, bytewise;  // bytewise: the command copy's form (fpx_epx_cmds.hpp)
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;  // [m + 1]
  uint8_t* reply_kind;   // [m]
  int64_t* totals;       // [4]: encoded, bytes needed, deferred, the first unknown outcome (-1 = none)
  uint32_t* lscan;       // [rows * INTERN_ROW] the lengths, then their exclusive scan inside the row
  int32_t* ltot;         // [rows] the rows' sums, then their exclusive scan (32 bits: it wraps beyond 4 GiB)
  int32_t* lgt;          // [1] the total, 32 bits of it
  int32_t* ctl;          // [ERE_C_WORDS]: the first unknown outcome (atomicMin), 1 = emit, the two counts
};

__device__ __forceinline__ void ere_report(const EpxState& st, int code, int index) {
  if (atomicCAS(&st.status[EPX_ST_ENC], 0, code) == 0) st.status[EPX_ST_ENC_INDEX] = index;
}

// (the grid covers the records padded to whole rows of the scan: the padding counts as zero)
__global__ void __launch_bounds__(ERE_BLOCK) k_ere_len(const EreArgs a) {
  const int32_t i = blockIdx.x * ERE_BLOCK + threadIdx.x;
  uint32_t bytes = 0;
  int kind = fpxw::EPX_REPLY_NONE;
  if (i < a.m) {
    const fpxw::EpxReplyPlan p = fpxw::epx_reply_plan(a.in, i);
    if (p.kind == fpxw::EPX_REPLY_UNKNOWN) atomicMin(&a.ctl[ERE_C_BAD], i);
    bytes = (uint32_t)p.len, kind = p.kind;
  }
  a.lscan[i] = bytes;
  const unsigned long long enc = __ballot(kind == fpxw::EPX_REPLY_ENCODED), def = __ballot(kind == fpxw::EPX_REPLY_DEFERRED);
  if ((threadIdx.x & 63) == 0) {
    if (enc) atomicAdd(&a.ctl[ERE_C_ENCODED], __popcll(enc));
    if (def) atomicAdd(&a.ctl[ERE_C_DEFERRED], __popcll(def));
  }
}

// a context in its "apply nothing" state (a refused burst in front of this call): its records mean nothing
__device__ __forceinline__ bool ere_refused(const EpxState& st) {
  const int32_t s = st.status[0];
  return s != 0 && s != FPX_EFATAL_PROTOCOL;
}

// behind the two levels of the scan.  ltot[j] is the rows' exclusive scan modulo 2^32 and a row's sum is far below 2^32 (1024
// replies of at most 2^16 bytes of command and a few hundred more), so neighbours' differences are the rows' sums exactly and their 64-bit sum is the
// bytes needed, however large
__global__ void __launch_bounds__(256) k_ere_decide(const EpxState st, const EreArgs a) {
  __shared__ unsigned long long bytes_all;
  if (threadIdx.x == 0) bytes_all = 0;
  __syncthreads();
  const bool refused = ere_refused(st);  // (the scans stood back behind an FPX_EINVAL: their words are read only when the status is clean)
  if (!refused) {
    unsigned long long mine = 0;
    for (int32_t j = threadIdx.x; j < a.rows; j += 256)
      mine += (uint32_t)((j + 1 < a.rows ? (uint32_t)a.ltot[j + 1] : (uint32_t)*a.lgt) - (uint32_t)a.ltot[j]);
    if (mine) atomicAdd(&bytes_all, mine);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int32_t bad = a.ctl[ERE_C_BAD];
  const unsigned long long bytes = bytes_all;
  int go = 0;
  a.out_offsets[0] = 0;
  a.totals[0] = a.totals[1] = a.totals[2] = 0, a.totals[3] = -1;
  if (refused) {
    // nothing is encoded either
  } else if (bad != ERE_NO_BAD) {
    a.totals[3] = bad;
    ere_report(st, FPX_EINVAL, bad);
  } else {
    a.totals[0] = a.ctl[ERE_C_ENCODED], a.totals[1] = (int64_t)bytes, a.totals[2] = a.ctl[ERE_C_DEFERRED];
    if ((int64_t)bytes > a.cap || bytes > 0xffffffffull) ere_report(st, FPX_ECAPACITY, -1);
    else go = 1;
  }
  a.ctl[ERE_C_GO] = go;
}

// the record of the wavefront that holds byte pos of its span: rel[lo] <= pos < rel[lo + 1] (rel[0] = 0, rel[64] > pos is
// the caller's; records without bytes are stepped over)
__device__ __forceinline__ int ere_find(const int32_t* rel, int32_t pos) {
  int lo = 0, hi = 64;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rel[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(ERE_BLOCK) k_ere_emit(const EreArgs a) {
  __shared__ int32_t rel[ERE_BLOCK / 64][65];
  __shared__ uint8_t slot[ERE_BLOCK / 64][64][ERE_SLOT];
  if (a.ctl[ERE_C_GO] == 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * ERE_BLOCK + threadIdx.x;
  fpxw::EpxReplyPlan p{fpxw::EPX_REPLY_NONE, 0, 0};
  if (i < a.m) p = fpxw::epx_reply_plan(a.in, i);
  const uint64_t len = (uint64_t)p.len;
  // (a lane past m reads the padding of its row: the row's sum so far, where the wavefront's span ends)
  const uint64_t off = (uint64_t)(uint32_t)(a.lscan[i] + (uint32_t)a.ltot[i / (int32_t)INTERN_ROW]);
  if (i < a.m) {
    a.out_offsets[i] = (int64_t)off;
    a.reply_kind[i] = (uint8_t)p.kind;
    if (i == a.m - 1) a.out_offsets[a.m] = (int64_t)(off + len);
  }
  const bool enc = p.kind == fpxw::EPX_REPLY_ENCODED;
  const bool cmd = enc && p.cmd_len >= 0;
  const bool direct = a.direct != 0 || __any(len > (uint64_t)ERE_SLOT || cmd) != 0;  // the same in every lane of the wavefront
  int64_t cmd_at = 0;
  if (cmd) (void)fpxw::epx_reply_emit_around(a.out + off, a.in, i, p, &cmd_at);
  else if (enc) (void)fpxw::epx_reply_emit(direct ? a.out + off : slot[wave][lane], a.in, i, p.outcome);
  // the commands of the wavefront, one after the other, all 64 lanes on each
  for (unsigned long long has = __ballot(cmd && p.cmd_len > 0); has; has &= has - 1) {
    const int l = __ffsll((long long)has) - 1;
    uint8_t* const dst = a.out + __shfl((long long)(off + (uint64_t)cmd_at), l);
    const uint8_t* const src = a.in.cmds.arena + __shfl((long long)p.cmd_off, l);
    cmds_wave_copy(dst, CmdOneRun{src, __shfl(p.cmd_len, l)}, lane, a.bytewise != 0);
  }
  const int64_t s = __shfl((long long)off, 0), e = __shfl((long long)(off + len), 63);
  rel[wave][lane] = (int32_t)((int64_t)off - s);
  if (lane == 63) rel[wave][64] = (int32_t)(e - s);
  __syncthreads();
  if (direct) return;
  // the span [0, total) of this wavefront, relative to out + s, cut at 16-byte boundaries of the output ADDRESS
  const int32_t* r = rel[wave];
  const int32_t total = r[64];
  uint8_t* const base = a.out + s;
  const int32_t first = -(int32_t)((uintptr_t)base & 15);  // may lie before 0: only [0, total) is touched
  for (int32_t c = first + lane * 16; c < total; c += 64 * 16) {
    const int k0 = c < 0 ? -c : 0, k1 = total - c < 16 ? total - c : 16;
    uint64_t v[2] = {0, 0};
    int rec = ere_find(r, c + k0);
    for (int k = k0; k < k1; ++k) {
      const int32_t pos = c + k;
      while (pos >= r[rec + 1]) ++rec;
      v[k >> 3] |= (uint64_t)slot[wave][rec][pos - r[rec]] << ((k & 7) * 8);
    }
    if (k0 == 0 && k1 == 16) {
      typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
      u64x2 q;
      q.x = v[0], q.y = v[1];
      *reinterpret_cast<u64x2*>(base + c) = q;
    } else {  // the ragged ends of the span: its neighbours own the rest of these sixteen bytes
      for (int k = k0; k < k1; ++k) base[c + k] = (uint8_t)(v[k >> 3] >> ((k & 7) * 8));
    }
  }
}
