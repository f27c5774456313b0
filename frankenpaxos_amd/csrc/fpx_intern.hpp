// fpx_intern.hpp -- a device table that interns byte strings: equal strings get equal ids, new strings the ids count,
// count + 1, ... in order of FIRST OCCURRENCE in the batch, so the ids are a function of the input alone, whatever the
// schedule.  It is the EPaxos context's key table (include/fpx.h, fpx_epx_keys_*): what GpuEPaxosEngine.keyOf
// (jni/EPaxosNative.scala) is on the JVM.  Included by fpx_epaxos.hip inside its anonymous namespace; the hash alone is
// host code too (fpx_wire.cpp exports it for the tests).
//
// State: `slots` 64-bit slot words (a power of two >= 2 x num_keys, at least 16): state << 32 | payload, state EMPTY /
// PENDING / RESIDENT, payload the claiming pair's index while pending and the id once resident; first[slots] (idle:
// INTERN_IDLE); key_off[num_keys + 1], the byte offsets of the interned keys by id; the byte arena; meta = {count,
// arena_used}.  Open addressing, linear probing, no deletion: the table only grows.
//
// A batch is P strings (off, len) of a byte buffer, in launches of their own (a kernel boundary is the only hand-off here):
//   k_int_probe     one thread per string: FNV-1a 64 picks the home slot and nothing else; identity is the byte compare,
//                   against the arena at a resident slot and against the INPUT bytes of the claiming pair at a pending one
//                   (no thread writes the input in this launch).  An empty slot is claimed by compare-and-swap; every
//                   thread that ends on a pending slot does atomicMin(first[slot], own index).  No thread waits for
//                   another: the only loop is the probe, at most `slots` steps.
//   k_int_flags     pair p is the first occurrence of a new string iff its slot is pending and first[slot] == p; the
//                   flags and the flagged lengths as arrays
//   k_lr_bscan      (fpx_epx_leader.hpp: scan_array_excl of fpx_scan.hpp, a workgroup per row) twice per array: the
//                   exclusive scan inside every row of 1024 pairs with the rows' sums, then the scan of those sums
//   k_int_decide    the totals and the decision: a bad string, an error already raised on the context, count + new >
//                   num_keys, arena_used + new bytes > arena_bytes or a probe that found no slot -> the batch applies
//                   nothing
//   k_int_rollback  (refused batches) every pending slot back to empty, first[] back to idle.  Safe under linear probing:
//                   resident entries were all inserted in earlier batches, so no resident chain runs through a pending slot
//   k_int_commit    (applied batches) a first occurrence writes key_off, copies its bytes into the arena, sets first[] back
//                   to idle and stores (RESIDENT, id) into its slot
//   k_int_ids       every pair reads its slot's id (-1 in a refused batch)
// Memory model: slot words and first[] are touched with agent-scope atomics only, relaxed loads included -- another CU's
// L1 may hold a stale copy of a line a plain load would hit.  Arena bytes and key_off are read only in launches after the
// one that wrote them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FPX_INTERN_HD __host__ __device__
#else
#define FPX_INTERN_HD
#endif

namespace fpxi {

constexpr int32_t KEY_MAX_LEN = 4096;  // FPX_EPX_KEY_MAX_LEN

// FNV-1a, 64 bits
FPX_INTERN_HD inline uint64_t fnv1a64(const uint8_t* p, int64_t len) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t j = 0; j < len; ++j) h = (h ^ p[j]) * 0x100000001b3ull;
  return h;
}

// the slot words of a table of num_keys ids
inline int32_t slots_for(int32_t num_keys) {
  int32_t s = 16;
  while (s < 2 * (int64_t)num_keys) s <<= 1;
  return s;
}

}  // namespace fpxi

#if defined(__HIPCC__)

constexpr int32_t INTERN_IDLE = 0x7f7f7f7f;  // above every pair index, and one byte four times: a memset makes it
constexpr uint32_t INTERN_EMPTY = 0, INTERN_PENDING = 1, INTERN_RESIDENT = 2;
constexpr int INTERN_ROW = 1024;  // what one workgroup of the array scan takes: fpx::INTERN_SCAN_ROW
// control words of a batch (int64): zeroed before the probe
enum { IC_NEW = 0, IC_NEW_BYTES = 1, IC_BAD = 2 /* 0x7fffffff - lowest bad index, 0 = none */, IC_OVERFLOW = 3, IC_APPLY = 4,
       IC_BASE_COUNT = 5, IC_BASE_BYTES = 6, IC_WORDS = 8 };

struct InternTable {
  unsigned long long* slot;
  int32_t* first;
  int32_t* key_off;
  uint8_t* arena;
  int32_t* meta;  // count, arena_used
  int32_t slots, num_keys;
  int64_t arena_bytes;
};

struct InternBatch {
  const uint8_t* bytes;
  int64_t bytes_len;
  const int64_t* off;
  const int32_t* len;
  int32_t P;             // the pairs of the call, or their most when count is given
  const int32_t* count;  // null, or the device word that holds the number of pairs (<= P)
  int32_t* ids;
  // scratch of the call
  int32_t* slot_of;   // [P] the pair's slot; -1: a bad string, -2: no slot found
  int32_t* rank;      // [P] scratch of the flags
  uint32_t* sc[3];    // [P padded to rows of INTERN_ROW] flag, low and high half of the flagged length; then their scans
  int32_t* tot[3];    // [rows] the rows' sums, then their exclusive scans
  int32_t* gt;        // [4] the three totals
  long long* ctl;     // [IC_WORDS]
};

__device__ __forceinline__ int32_t intern_pairs(const InternBatch& b) {
  if (!b.count) return b.P;
  const int32_t c = *b.count;
  return c < 0 ? 0 : (c < b.P ? c : b.P);
}
__device__ __forceinline__ unsigned long long intern_load(const unsigned long long* w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool intern_same(const uint8_t* a, const uint8_t* b, int32_t len) {
  for (int32_t j = 0; j < len; ++j)
    if (a[j] != b[j]) return false;
  return true;
}

__global__ void __launch_bounds__(256) k_int_probe(const InternTable t, const InternBatch b) {
  const int32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= intern_pairs(b)) return;
  const int64_t off = b.off[p];
  const int32_t len = b.len[p];
  if (off < 0 || len < 0 || len > fpxi::KEY_MAX_LEN || off > b.bytes_len - len) {
    atomicMax((unsigned long long*)&b.ctl[IC_BAD], (unsigned long long)(0x7fffffff - p));
    b.slot_of[p] = -1;
    return;
  }
  const uint8_t* mine = b.bytes + off;
  const uint32_t mask = (uint32_t)t.slots - 1u;
  uint32_t s = (uint32_t)fpxi::fnv1a64(mine, len) & mask;
  int32_t found = -2;
  bool pending = false;
  for (int32_t step = 0; step < t.slots; ++step, s = (s + 1u) & mask) {
    unsigned long long w = intern_load(&t.slot[s]);
    if ((uint32_t)(w >> 32) == INTERN_EMPTY) {
      const unsigned long long want = ((unsigned long long)INTERN_PENDING << 32) | (uint32_t)p;
      unsigned long long seen = 0;
      if (__hip_atomic_compare_exchange_strong(&t.slot[s], &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        found = (int32_t)s, pending = true;
        break;
      }
      w = seen;  // someone else's claim: a pending word (nothing becomes resident in this launch)
    }
    const uint32_t state = (uint32_t)(w >> 32), payload = (uint32_t)w;
    if (state == INTERN_RESIDENT) {
      const int32_t at = t.key_off[payload];
      if (t.key_off[payload + 1] - at == len && intern_same(mine, t.arena + at, len)) {
        found = (int32_t)s;
        break;
      }
    } else if (b.len[payload] == len && intern_same(mine, b.bytes + b.off[payload], len)) {
      found = (int32_t)s, pending = true;
      break;
    }
  }
  if (found == -2) atomicMax((unsigned long long*)&b.ctl[IC_OVERFLOW], 1ull);
  else if (pending) atomicMin(&t.first[found], p);
  b.slot_of[p] = found;
}

// is pair p (slot sl) the first occurrence of a new string?
__device__ __forceinline__ bool intern_is_first(const InternTable& t, int32_t p, int32_t sl) {
  if (sl < 0) return false;
  if ((uint32_t)(intern_load(&t.slot[sl]) >> 32) != INTERN_PENDING) return false;
  return __hip_atomic_load(&t.first[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p;
}

// the flags, and what the scans run over: per pair its flag and its flagged length as two halves (low 6 bits, the rest: a
// key has at most 4096 bytes and a batch 2^23 pairs, so neither half's sum leaves 32 bits).  The grid covers the pairs
// padded to whole rows of INTERN_ROW: the padding scans as zeros
__global__ void __launch_bounds__(256) k_int_flags(const InternTable t, const InternBatch b) {
  const int32_t p = blockIdx.x * 256 + threadIdx.x;
  const bool in = p < intern_pairs(b);
  const bool flag = in && intern_is_first(t, p, b.slot_of[p]);
  if (in) b.rank[p] = flag;
  const uint32_t len = flag ? (uint32_t)b.len[p] : 0u;
  b.sc[0][p] = flag, b.sc[1][p] = len & 63u, b.sc[2][p] = len >> 6;
}

// one thread, behind the scans.  st_status: the context's status words (an error raised in front refuses the batch; the
// scan kernels stand back behind an FPX_EINVAL, so the totals are read only when the status is clean)
__global__ void k_int_decide(const InternTable t, const InternBatch b, int32_t* st_status) {
  const int32_t count = t.meta[0], used = t.meta[1];
  const long long bad = b.ctl[IC_BAD];
  long long fresh = 0, fresh_bytes = 0;
  int code = 0, index = -1;
  if (st_status[0] != 0) {
    code = st_status[0];  // (already raised: reported by whoever raised it)
  } else {
    fresh = b.P > 0 ? b.gt[0] : 0, fresh_bytes = b.P > 0 ? ((long long)b.gt[2] << 6) + b.gt[1] : 0;
    if (bad != 0) code = FPX_EINVAL, index = (int32_t)(0x7fffffff - bad);
    else if (b.ctl[IC_OVERFLOW] != 0 || count + fresh > t.num_keys || used + fresh_bytes > t.arena_bytes) code = FPX_ECAPACITY;
    if (code != 0) epx_report(st_status, code, index);
  }
  b.ctl[IC_APPLY] = code == 0;
  b.ctl[IC_NEW] = code == 0 ? fresh : 0, b.ctl[IC_NEW_BYTES] = code == 0 ? fresh_bytes : 0;
  b.ctl[IC_BASE_COUNT] = count, b.ctl[IC_BASE_BYTES] = used;
  if (code == 0) t.meta[0] = count + (int32_t)fresh, t.meta[1] = used + (int32_t)fresh_bytes;
}

__global__ void __launch_bounds__(256) k_int_rollback(const InternTable t, const InternBatch b) {
  if (b.ctl[IC_APPLY]) return;
  const int32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= intern_pairs(b)) return;
  const int32_t sl = b.slot_of[p];
  if (sl < 0 || (uint32_t)(intern_load(&t.slot[sl]) >> 32) != INTERN_PENDING) return;
  // (every pair of the slot stores the same two words)
  __hip_atomic_store(&t.first[sl], INTERN_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&t.slot[sl], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_int_commit(const InternTable t, const InternBatch b) {
  if (!b.ctl[IC_APPLY]) return;
  const int32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= intern_pairs(b) || b.rank[p] == 0) return;
  // (sc: the exclusive scans inside the pair's row by now; tot: of the rows' sums.  An applied batch's bytes fit the arena)
  const int32_t row = p / INTERN_ROW, len = b.len[p];
  const int32_t id = (int32_t)b.ctl[IC_BASE_COUNT] + (int32_t)(b.sc[0][p] + (uint32_t)b.tot[0][row]);
  const uint32_t br = ((b.sc[2][p] + (uint32_t)b.tot[2][row]) << 6) + b.sc[1][p] + (uint32_t)b.tot[1][row];
  const int32_t at = (int32_t)(b.ctl[IC_BASE_BYTES] + br);
  const int32_t sl = b.slot_of[p];
  t.key_off[id + 1] = at + len;  // (key_off[0] = 0 since the table was made; id's start is id - 1's end)
  const uint8_t* src = b.bytes + b.off[p];
  for (int32_t j = 0; j < len; ++j) t.arena[at + j] = src[j];
  __hip_atomic_store(&t.first[sl], INTERN_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&t.slot[sl], ((unsigned long long)INTERN_RESIDENT << 32) | (uint32_t)id, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// P here is the grid's bound, not the device count: a refused batch writes -1 for every pair the caller sized
__global__ void __launch_bounds__(256) k_int_ids(const InternTable t, const InternBatch b) {
  const int32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= intern_pairs(b)) return;
  const int32_t sl = b.slot_of[p];
  b.ids[p] = b.ctl[IC_APPLY] && sl >= 0 ? (int32_t)(uint32_t)intern_load(&t.slot[sl]) : -1;
}

#endif  // __HIPCC__
