// fpx_epx_cmds.hpp -- the EPaxos context's command store (include/fpx.h, fpx_epx_cmds_*): the serialised CommandOrNoop of a
// triple, by triple id, on the device -- what engine.triples (jni/EPaxosNative.scala) is on the JVM.  With it the replies
// that carry a stored command (the Commit sent back, the PrepareOk of a seen instance) are encoded on the device too
// (fpx_wire_epx_enc_dev.hpp).  Included by fpx_epaxos.hip inside its anonymous namespace.
//
// State: off[max_triples] (64-bit arena offset, -1 = no bytes), len[max_triples], claim[max_triples] (idle between
// calls: CMDS_IDLE), the byte arena, which only grows, and meta[4] = {commands stored, arena bytes used, records skipped,
// bursts refused}.
//
// A burst is m records (cmd_off, cmd_len, triple_id) over a byte buffer.  Record i is CONSIDERED iff triple_id[i] >= 0 and
// cmd_len[i] >= 0; a considered record whose id is >= max_triples or whose length is above CMD_MAX_LEN is SKIPPED (counted,
// no error); an id that has bytes already is left alone (first stored wins, nothing is compared); among the remaining
// records of one id the lowest index is the WRITER.  The writers' commands go into the arena in index order, without
// padding, so the arena is a function of the input alone, whatever the schedule.  In launches of their own (a kernel
// boundary is the only hand-off here):
//   k_cmd_claim   one thread per record: the span check (standalone call only), the skip count, atomicMin(claim[id], i)
//   k_cmd_len     the writers' lengths as the element of the scan (everyone else 0), the writers' count
//   k_lr_bscan    (fpx_epx_leader.hpp) twice: the exclusive scan inside rows of 1024 records, then of the rows' sums; 32 bits
//   k_cmd_decide  ONE workgroup: the new bytes as a 64-bit sum of the rows' sums; a bad span (FPX_EINVAL on the context), a
//                 burst that does not fit the free arena or reaches 4 GiB (a REFUSED burst: counted, no status), a status
//                 raised in front of the put (it stands back: nothing stored, nothing counted); result and meta
//   k_cmd_copy    an applied burst: off / len of the writers, and the bytes -- a wavefront copies the contiguous arena span
//                 of its 64 records cooperatively (cmds_wave_copy)
//   k_cmd_release the claim words of the burst back to idle, applied or not
// Memory model: claim words are touched with agent-scope atomics only; off, len and the arena are read only in launches
// after the one that wrote them.
//
// cmds_wave_copy is the copy of both users, this store and the reply encoder (one command, all 64 lanes on it).  Two forms,
// A/B in profiles/epx_wire_replica_cmds.md -- on commands of 24 bytes the single-byte form won in the put, in the encoder
// (2 x) and in the recovery tick, so it is the default and the word form stays behind FPX_EPX_CMDS_WORDS (in the environment
// of fpx_epx_create) for callers with long commands:
//   words  the destination span is cut at 16-byte boundaries of its ADDRESS; lane l takes piece l, l + 64, ...  A whole
//          piece that lies inside one record is one unaligned 16-byte load and one aligned 16-byte store; a piece that
//          crosses records is assembled byte by byte and stored as one word; single bytes only at the ragged ends
//   bytes  lane l takes byte l, l + 64, ...: coalesced single-byte copies
// wave64; plain C++ vector stores only.
#pragma once
#include <stdint.h>

constexpr int32_t CMD_MAX_LEN = 1 << 16;     // FPX_EPX_CMD_MAX_LEN
constexpr int32_t CMDS_IDLE = 0x7f7f7f7f;    // above every record index, and one byte four times: a memset makes it
constexpr int CMD_BLOCK = 256;               // records per workgroup
enum { CMC_BAD = 0 /* lowest bad index, CMDS_IDLE = none */, CMC_GO = 1, CMC_NEW = 2, CMC_SKIPPED = 3, CMC_BASE = 4 /* 64 bits */,
       CMC_WORDS = 8 };
enum { CMM_COUNT = 0, CMM_USED = 1, CMM_SKIPPED = 2, CMM_REFUSED = 3 };

struct CmdStore {
  long long* off;   // [max_triples]
  int32_t* len;     // [max_triples]
  int32_t* claim;   // [max_triples]
  uint8_t* arena;
  long long* meta;  // [4]
  int32_t max_triples;
  int64_t arena_bytes;
};

struct CmdPut {
  const uint8_t* buf;
  int64_t buf_len;
  const int64_t* cmd_off;
  const int32_t* cmd_len;
  const int32_t* triple;
  int32_t m, rows, check_spans, bytewise;
  long long* result;  // [4] new commands, new bytes, skipped, refused (may be null)
  uint32_t* lscan;    // [rows * INTERN_ROW] the writers' lengths, then their exclusive scan inside the row
  int32_t* ltot;      // [rows]
  int32_t* lgt;       // [1]
  int32_t* ctl;       // [CMC_WORDS]
};

// the records of a copy, by the bytes they put into the span: rel(k) is where record k starts (rel(count()) the span's
// length), src(k) its bytes.  A record may be empty
struct CmdOneRun {
  const uint8_t* p;
  int32_t len;
  __device__ __forceinline__ int count() const { return 1; }
  __device__ __forceinline__ int32_t rel(int k) const { return k ? len : 0; }
  __device__ __forceinline__ const uint8_t* src(int) const { return p; }
};
struct CmdWaveRuns {
  const int32_t* r;             // [65] LDS
  const uint8_t* const* s;      // [64] LDS
  __device__ __forceinline__ int count() const { return 64; }
  __device__ __forceinline__ int32_t rel(int k) const { return r[k]; }
  __device__ __forceinline__ const uint8_t* src(int k) const { return s[k]; }
};

// the record that holds byte pos of the span: the largest k with rel(k) <= pos (pos < rel(count()) is the caller's)
template <typename R>
__device__ __forceinline__ int cmds_find(const R& recs, int32_t pos) {
  int lo = 0, hi = recs.count();
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (recs.rel(mid) <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// all 64 lanes of a wavefront copy the records' bytes, back to back, to base[0 .. rel(count()))
template <typename R>
__device__ __forceinline__ void cmds_wave_copy(uint8_t* base, const R& recs, int lane, bool bytewise) {
  const int32_t total = recs.rel(recs.count());
  if (total <= 0) return;
  if (bytewise) {
    if (lane >= total) return;
    int rec = cmds_find(recs, lane);
    for (int32_t pos = lane; pos < total; pos += 64) {
      while (pos >= recs.rel(rec + 1)) ++rec;
      base[pos] = recs.src(rec)[pos - recs.rel(rec)];
    }
    return;
  }
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  const int32_t first = -(int32_t)((uintptr_t)base & 15);  // may lie before 0: only [0, total) is touched
  for (int32_t c = first + lane * 16; c < total; c += 64 * 16) {
    const int k0 = c < 0 ? -c : 0, k1 = total - c < 16 ? total - c : 16;
    int rec = cmds_find(recs, c + k0);
    if (k0 == 0 && k1 == 16 && c + 16 <= recs.rel(rec + 1)) {  // a whole piece of one record
      u64x2 q;
      __builtin_memcpy(&q, recs.src(rec) + (c - recs.rel(rec)), 16);
      *reinterpret_cast<u64x2*>(base + c) = q;
      continue;
    }
    uint64_t v[2] = {0, 0};
    for (int k = k0; k < k1; ++k) {
      const int32_t pos = c + k;
      while (pos >= recs.rel(rec + 1)) ++rec;
      v[k >> 3] |= (uint64_t)recs.src(rec)[pos - recs.rel(rec)] << ((k & 7) * 8);
    }
    if (k0 == 0 && k1 == 16) {
      u64x2 q;
      q.x = v[0], q.y = v[1];
      *reinterpret_cast<u64x2*>(base + c) = q;
    } else {  // the ragged ends of the span: its neighbours own the rest of these sixteen bytes
      for (int k = k0; k < k1; ++k) base[c + k] = (uint8_t)(v[k >> 3] >> ((k & 7) * 8));
    }
  }
}

// a context in its "apply nothing" state: the put stands back
__device__ __forceinline__ bool cmds_stand_back(const EpxState& st) {
  const int32_t s = st.status[0];
  return s != 0 && s != FPX_EFATAL_PROTOCOL;
}

// what record i is: -1 not considered or skipped, else its triple id (in range)
__device__ __forceinline__ int32_t cmds_id(const CmdStore& t, const CmdPut& b, int32_t i, bool* skipped) {
  const int32_t id = b.triple[i], len = b.cmd_len[i];
  *skipped = false;
  if (id < 0 || len < 0) return -1;
  if (id >= t.max_triples || len > CMD_MAX_LEN) {
    *skipped = true;
    return -1;
  }
  return id;
}
__device__ __forceinline__ int32_t cmds_claim_load(const int32_t* w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(CMD_BLOCK) k_cmd_claim(const EpxState st, const CmdStore t, const CmdPut b) {
  const int32_t i = blockIdx.x * CMD_BLOCK + threadIdx.x;
  if (cmds_stand_back(st)) return;
  bool skipped = false;
  int32_t id = -1;
  if (i < b.m) {
    id = cmds_id(t, b, i, &skipped);
    if (b.check_spans && b.triple[i] >= 0 && b.cmd_len[i] >= 0) {
      const int64_t off = b.cmd_off[i];
      if (off < 0 || off > b.buf_len - (int64_t)b.cmd_len[i]) atomicMin(&b.ctl[CMC_BAD], i), id = -1, skipped = false;
    }
    if (id >= 0 && t.off[id] < 0) atomicMin(&t.claim[id], i);
  }
  const unsigned long long sk = __ballot(skipped);
  if ((threadIdx.x & 63) == 0 && sk) atomicAdd(&b.ctl[CMC_SKIPPED], __popcll(sk));
}

// is record i the writer of its id?
__device__ __forceinline__ bool cmds_is_writer(const CmdStore& t, const CmdPut& b, int32_t i) {
  bool skipped;
  const int32_t id = cmds_id(t, b, i, &skipped);
  return id >= 0 && t.off[id] < 0 && cmds_claim_load(&t.claim[id]) == i;
}

// (the grid covers the records padded to whole rows of the scan: the padding counts as zero)
__global__ void __launch_bounds__(CMD_BLOCK) k_cmd_len(const EpxState st, const CmdStore t, const CmdPut b) {
  const int32_t i = blockIdx.x * CMD_BLOCK + threadIdx.x;
  const bool writer = i < b.m && !cmds_stand_back(st) && cmds_is_writer(t, b, i);
  b.lscan[i] = writer ? (uint32_t)b.cmd_len[i] : 0u;
  const unsigned long long wr = __ballot(writer);
  if ((threadIdx.x & 63) == 0 && wr) atomicAdd(&b.ctl[CMC_NEW], __popcll(wr));
}

// behind the two levels of the scan.  ltot[j] is the rows' exclusive scan modulo 2^32 and a row's sum is at most 1024 x 2^16,
// so neighbours' differences are the rows' sums exactly and their 64-bit sum is the new bytes, however many
__global__ void __launch_bounds__(256) k_cmd_decide(const EpxState st, const CmdStore t, const CmdPut b) {
  __shared__ unsigned long long bytes_all;
  if (threadIdx.x == 0) bytes_all = 0;
  __syncthreads();
  const bool back = cmds_stand_back(st);  // (the scans stood back behind an FPX_EINVAL: their words are read only when the status is clean)
  if (!back) {
    unsigned long long mine = 0;
    for (int32_t j = threadIdx.x; j < b.rows; j += 256)
      mine += (uint32_t)((j + 1 < b.rows ? (uint32_t)b.ltot[j + 1] : (uint32_t)*b.lgt) - (uint32_t)b.ltot[j]);
    if (mine) atomicAdd(&bytes_all, mine);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int32_t bad = b.ctl[CMC_BAD];
  const long long bytes = (long long)bytes_all, used = t.meta[CMM_USED];
  long long res[4] = {0, 0, 0, 0};
  int go = 0;
  if (back) {
    // nothing is stored and nothing is counted
  } else if (bad != CMDS_IDLE) {
    res[0] = -1, res[1] = bad;
    epx_report(st.status, FPX_EINVAL, bad);
  } else {
    res[2] = b.ctl[CMC_SKIPPED];
    t.meta[CMM_SKIPPED] += res[2];
    if (bytes > t.arena_bytes - used || bytes > 0xffffffffll) {
      res[3] = 1;
      t.meta[CMM_REFUSED] += 1;
    } else {
      res[0] = b.ctl[CMC_NEW], res[1] = bytes, go = 1;
      t.meta[CMM_COUNT] += res[0], t.meta[CMM_USED] = used + bytes;
    }
  }
  if (b.result)
    for (int k = 0; k < 4; ++k) b.result[k] = res[k];
  b.ctl[CMC_GO] = go;
  *reinterpret_cast<long long*>(&b.ctl[CMC_BASE]) = used;
}

__global__ void __launch_bounds__(CMD_BLOCK) k_cmd_copy(const CmdStore t, const CmdPut b) {
  __shared__ int32_t rel[CMD_BLOCK / 64][65];
  __shared__ const uint8_t* src[CMD_BLOCK / 64][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * CMD_BLOCK + threadIdx.x;
  const bool go = b.ctl[CMC_GO] != 0;
  bool skipped, writer = false;
  int32_t id = -1, len = 0;
  if (go && i < b.m) {
    id = cmds_id(t, b, i, &skipped);
    // (off[id] is written by the id's writer in THIS launch, so who writes is read from the claim word alone: an id that
    // had bytes was never claimed, its word is idle)
    writer = id >= 0 && cmds_claim_load(&t.claim[id]) == i;
    if (writer) len = b.cmd_len[i];
  }
  // (a lane past m reads the padding of its row: the row's sum so far, where the wavefront's span ends)
  const uint64_t at = (uint64_t)(uint32_t)(b.lscan[i] + (uint32_t)b.ltot[i / (int32_t)INTERN_ROW]);
  const int64_t s = __shfl((long long)at, 0), e = __shfl((long long)(at + (uint64_t)len), 63);
  rel[wave][lane] = (int32_t)((int64_t)at - s);
  src[wave][lane] = writer ? b.buf + b.cmd_off[i] : nullptr;
  if (lane == 63) rel[wave][64] = (int32_t)(e - s);
  __syncthreads();
  const long long base = *reinterpret_cast<const long long*>(&b.ctl[CMC_BASE]);
  if (go) cmds_wave_copy(t.arena + base + s, CmdWaveRuns{rel[wave], src[wave]}, lane, b.bytewise != 0);
  if (writer) t.off[id] = base + (long long)at, t.len[id] = len;
}

// the claim words of the burst back to idle, in a launch of its own: k_cmd_copy reads them
__global__ void __launch_bounds__(CMD_BLOCK) k_cmd_release(const CmdStore t, const CmdPut b) {
  const int32_t i = blockIdx.x * CMD_BLOCK + threadIdx.x;
  if (i >= b.m) return;
  bool skipped;
  const int32_t id = cmds_id(t, b, i, &skipped);
  // (every record of an id stores the same word)
  if (id >= 0 && cmds_claim_load(&t.claim[id]) != CMDS_IDLE)
    __hip_atomic_store(&t.claim[id], CMDS_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
