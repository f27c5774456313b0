// fpx_wire_enc_dev.hpp -- the wire adapter's encoders on the device (include/fpx_wire.h, fpx_wire_encode_*_dev): the
// records a tick leaves in HBM (Chosen flags, vote bits, Nack rounds) become the serialised messages of the reply, back
// to back, with their offsets -- a stream compaction with variable-length output.  The bytes are fpx_wire_emit.hpp's,
// the source the host encoders compile, so the two agree by construction; tests/test_gpu_wire_encode.py holds them
// equal all the same.
//
// Three launches per call (profiles/wire_encode_dev.md has the argument against a single pass with chained look-back:
// its per-workgroup __threadfence is an L2 write-back on this multi-die part):
//   k_enc_len    one thread per record: the bytes and the messages it contributes; one sum of each per workgroup
//   k_enc_scan   ONE workgroup: exclusive scan of the workgroup sums, the totals, and the verdict (capacity, value spans)
//   k_enc_emit   one thread per record again: the record's place from a workgroup scan on top of its workgroup's base
//                (wave scan on the DPP network, the four wave totals through LDS), then each WAVEFRONT writes the span
//                of its 64 records
// The emit pass never stores single bytes to HBM except at the ragged ends of a wavefront's span.  The span is cut at
// 16-byte boundaries of the output ADDRESS; lane l assembles the sixteen bytes of piece l, l + 64, ... in registers --
// it finds the message a byte belongs to by a binary search over the 65 offsets the wavefront keeps in LDS, takes head
// bytes from the heads the 64 lanes emitted into LDS and value bytes from where the decoder found them -- and stores
// one aligned 16-byte word.  A piece that lies inside one value is ONE unaligned 16-byte load; a long value is thus
// copied by the whole wavefront, sixteen bytes a lane, whatever its alignment.
#pragma once
#include "fpx_kernels.hpp"
#include "fpx_wire_emit.hpp"

namespace fpx {

enum { ENC_CHOSEN = 0, ENC_PHASE2B = 1, ENC_NACK = 2 };
constexpr int ENC_BLOCK = 256;  // records per workgroup
constexpr int ENC_HEAD = 24;    // LDS bytes per head: CHOSEN_HEAD_MAX is 23 (a Noop's two value bytes ride in the head; its length varint is then one byte)
constexpr int ENC_MSG = 48;     // LDS bytes per generated Phase2b (PHASE2B_MAX = 46)
constexpr int32_t ENC_NO_BAD = 0x7f7f7f7f;  // (what a one-byte memset leaves: above any record index)

// scratch words (int64) of one call: [0] low half: the first record with a bad value span (atomicMin), [1] 1 = emit,
// then nblk workgroup byte sums and nblk workgroup message sums, scanned in place by k_enc_scan
enum { ENC_W_BAD = 0, ENC_W_GO = 1, ENC_W_SUMS = 2 };

struct EncArgs {
  int32_t n, nblk, dialect, grid_cols;
  const uint8_t* emit;      // Chosen: which records (null = all)
  const int32_t* slot;
  const int32_t* round;     // Phase2b; Nack: the Nack rounds (a record with round < 0 emits nothing)
  const int32_t* is_noop;   // Chosen (null = none)
  const uint8_t* values;    // Chosen
  int64_t values_len;
  const int64_t* value_off;
  const int32_t* value_len;
  const uint64_t* vote_bits;  // Phase2b: n x 4
  const int32_t* group_of_slot;
  uint8_t* out;
  int64_t cap, max_msgs;
  int64_t* out_offsets;
  int64_t* totals;
  int64_t* scratch;
};

// ---- wave64 inclusive sum of one 64-bit value per lane on the DPP network (kp_wave_excl_sum's steps; the two halves of
// the source lane's value travel as two moves, the addition is 64 bits wide) ----------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int64_t enc_dpp64(int64_t v) {
  const uint32_t lo = (uint32_t)dpp_or0<CTRL, ROW_MASK>((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)dpp_or0<CTRL, ROW_MASK>((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t enc_wave_incl_sum(int64_t v) {
  v += enc_dpp64<0x111, 0xF>(v);  // row_shr:1
  v += enc_dpp64<0x112, 0xF>(v);  // row_shr:2
  v += enc_dpp64<0x114, 0xF>(v);  // row_shr:4
  v += enc_dpp64<0x118, 0xF>(v);  // row_shr:8
  v += enc_dpp64<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v += enc_dpp64<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

// ---- one record ------------------------------------------------------------------------------------------------
// A record with a head and (Chosen) a value behind it
struct EncHv {
  int32_t emitted = 0, is_noop = 0, slot = 0, vlen = 0;  // vlen: the value's length as the message states it
  int64_t voff = 0, bytes = 0;
  bool bad = false;
};
template <int KIND>
__device__ __forceinline__ EncHv enc_hv(const EncArgs& a, int32_t i) {
  EncHv r;
  if (i >= a.n) return r;
  if (KIND == ENC_NACK) {
    r.slot = a.round[i];
    r.emitted = r.slot >= 0;
    if (r.emitted) r.bytes = fpxw::nack_len(r.slot);
    return r;
  }
  r.emitted = !a.emit || a.emit[i] != 0;
  if (!r.emitted) return r;
  r.slot = a.slot[i];
  r.is_noop = a.is_noop && a.is_noop[i] != 0;
  if (r.is_noop) {
    r.vlen = 2;
  } else {
    r.vlen = a.value_len[i] < 0 ? 0 : a.value_len[i];  // (as the host encoder's pick_value)
    r.voff = a.value_off[i];
    r.bad = r.voff < 0 || r.voff > a.values_len || (int64_t)r.vlen > a.values_len - r.voff;
    if (r.bad) {
      r.emitted = 0;
      return r;
    }
  }
  r.bytes = fpxw::chosen_len(r.slot, r.vlen);
  return r;
}

// The Phase2b's of one record.  bit -> (group_index, acceptor_index) as fpx_wire_encode_phase2b_batch maps it; a
// message's length depends on its bit only through the varints of those two, which are constant on each of four
// ranges of bits -- [0, 128), [128, c1), [c1, c2), [c2, 256) with c1 = grid_cols, c2 = grid_cols + 128 for a grid of
// more than 128 columns and c1 = c2 = 256 otherwise -- so the record's total is four popcounts times four lengths
struct EncP2b {
  int32_t slot, round, g0, cols, dialect;
  uint64_t w[4];
  int32_t cnt[4], len[4], lo[5];
  __device__ __forceinline__ void fields(int bit, int32_t* g, int32_t* a) const {
    *g = cols > 0 ? bit / cols : g0;
    *a = cols > 0 ? bit % cols : bit;
  }
  __device__ __forceinline__ int64_t count() const { return (int64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3]; }
  __device__ __forceinline__ int64_t bytes() const {
    return (int64_t)cnt[0] * len[0] + cnt[1] * len[1] + cnt[2] * len[2] + cnt[3] * len[3];
  }
  // message j of the record (j-th set bit): its offset from the record's first byte
  __device__ __forceinline__ int32_t offset_of(int32_t j) const {
    int32_t acc = 0;
    for (int r = 0; r < 3; ++r) {
      if (j < cnt[r]) return acc + j * len[r];
      acc += cnt[r] * len[r], j -= cnt[r];
    }
    return acc + j * len[3];
  }
  // the message that holds byte `rel` of the record: its index, first byte and length
  __device__ __forceinline__ void at(int32_t rel, int32_t* j, int32_t* start, int32_t* mlen) const {
    int32_t acc = 0, jb = 0, r = 0;
    for (; r < 3; ++r) {
      const int32_t span = cnt[r] * len[r];
      if (rel < span) break;
      acc += span, jb += cnt[r], rel -= span;
    }
    const int32_t k = rel / len[r];
    *j = jb + k, *start = acc + k * len[r], *mlen = len[r];
  }
  // the j-th set bit of the row
  __device__ __forceinline__ int select(int32_t j) const {
    int wd = 0;
    for (; wd < 3; ++wd) {
      const int c = __popcll(w[wd]);
      if (j < c) break;
      j -= c;
    }
    const uint64_t x = w[wd];
    int lo_bit = 0;
    for (int s = 32; s > 0; s >>= 1) {
      const int c = __popcll((x >> lo_bit) & ((1ull << s) - 1ull));
      if (j >= c) j -= c, lo_bit += s;
    }
    return wd * 64 + lo_bit;
  }
};
__device__ __forceinline__ EncP2b enc_p2b(const EncArgs& a, int32_t i) {
  EncP2b r;
  r.cols = a.grid_cols, r.dialect = a.dialect;
  r.lo[0] = 0, r.lo[1] = 128, r.lo[4] = 256;
  r.lo[2] = a.grid_cols > 128 && a.grid_cols < 256 ? a.grid_cols : 256;
  r.lo[3] = a.grid_cols > 128 && a.grid_cols + 128 < 256 ? a.grid_cols + 128 : 256;
  if (i >= a.n) {
    r.slot = r.round = r.g0 = 0;
    for (int k = 0; k < 4; ++k) r.w[k] = 0, r.cnt[k] = 0, r.len[k] = 1;
    return r;
  }
  r.slot = a.slot[i], r.round = a.round[i];
  r.g0 = a.grid_cols > 0 || !a.group_of_slot ? 0 : a.group_of_slot[i];
  for (int k = 0; k < 4; ++k) r.w[k] = a.vote_bits[(size_t)i * 4 + k];
  for (int k = 0; k < 4; ++k) {
    const int lo = r.lo[k], num = r.lo[k + 1] - lo;
    r.cnt[k] = 0;
    for (int wd = 0; wd < 4; ++wd) r.cnt[k] += __popcll(r.w[wd] & range_mask(lo, num, wd));
    int32_t g, ac;
    r.fields(lo < 256 ? lo : 255, &g, &ac);
    r.len[k] = (int32_t)fpxw::phase2b_len(a.dialect, g, ac, r.slot, r.round);
  }
  return r;
}

// ---- pass 1: lengths, one sum per workgroup -----------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(ENC_BLOCK) k_enc_len(const EncArgs a) {
  __shared__ int64_t wsum[2][4];
  const int32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x;
  int64_t bytes, count;
  if (KIND == ENC_PHASE2B) {
    const EncP2b r = enc_p2b(a, i);
    bytes = r.bytes(), count = r.count();
  } else {
    const EncHv r = enc_hv<KIND>(a, i);
    if (r.bad) atomicMin((int32_t*)&a.scratch[ENC_W_BAD], i);
    bytes = r.bytes, count = r.emitted;
  }
  bytes = enc_wave_incl_sum(bytes), count = enc_wave_incl_sum(count);
  if ((threadIdx.x & 63) == 63) wsum[0][threadIdx.x >> 6] = bytes, wsum[1][threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x < 2)
    a.scratch[ENC_W_SUMS + (size_t)threadIdx.x * a.nblk + blockIdx.x] =
        wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
}

// ---- pass 2: ONE workgroup scans the workgroup sums in place and decides -------------------------------------------
// The verdict is a per-call code (report, not report_abort): a reply that does not fit, or a value span that leaves the
// buffer, stops THIS encode -- the votes are applied already and the caller encodes again; later _dev calls go on.
__global__ void __launch_bounds__(1024) k_enc_scan(const State st, const EncArgs a) {
  __shared__ int64_t wtot[2][16];
  __shared__ int64_t carry[2];
  const int t = threadIdx.x, wave = t >> 6;
  if (t < 2) carry[t] = 0;
  __syncthreads();
  for (int32_t base = 0; base < a.nblk; base += 1024) {
    const int32_t b = base + t;
    int64_t v[2], inc[2];
    for (int k = 0; k < 2; ++k) {
      v[k] = b < a.nblk ? a.scratch[ENC_W_SUMS + (size_t)k * a.nblk + b] : 0;
      inc[k] = enc_wave_incl_sum(v[k]);
      if ((t & 63) == 63) wtot[k][wave] = inc[k];
    }
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
      int64_t before = carry[k];
      for (int w = 0; w < wave; ++w) before += wtot[k][w];
      if (b < a.nblk) a.scratch[ENC_W_SUMS + (size_t)k * a.nblk + b] = before + inc[k] - v[k];
    }
    __syncthreads();
    if (t < 2) {
      int64_t s = carry[t];
      for (int w = 0; w < 16; ++w) s += wtot[t][w];
      carry[t] = s;
    }
    __syncthreads();
  }
  if (t != 0) return;
  const int64_t bytes = carry[0], count = carry[1];
  const int32_t bad = a.nblk ? *(const int32_t*)&a.scratch[ENC_W_BAD] : ENC_NO_BAD;
  a.totals[0] = count, a.totals[1] = bytes;
  a.out_offsets[0] = 0;
  int go = 0;
  if (st.status[ST_ABORT] != 0) {
    // the run was refused (a bad tick, a contract violation): its records mean nothing, nothing is encoded
  } else if (bad != ENC_NO_BAD) {
    report(st, 1 /*FPX_EINVAL*/, bad, -1, -1);
  } else if (bytes > a.cap || count > a.max_msgs) {
    report(st, 5 /*FPX_ECAPACITY*/, -1, -1, -1);
  } else {
    go = 1;
    a.out_offsets[count] = bytes;
  }
  a.scratch[ENC_W_GO] = go;
}

// ---- pass 3 ----------------------------------------------------------------------------------------------------
// first index in [1, 64] whose entry is above pos, minus one: the record of the wavefront that holds byte (message) pos.
// off[64] > pos is the caller's; records that contribute nothing are stepped over
__device__ __forceinline__ int enc_find(const int64_t* off, int64_t pos) {
  int lo = 0, hi = 64;  // off[lo] <= pos < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// The wavefront's span [s, e) of the output: gen(pos, &ctx) -> the byte at pos, called with ascending pos inside one
// piece; whole(c, &v) (optional fast path) -> true if it produced all sixteen bytes of the piece at c itself.
template <typename Whole, typename Gen>
__device__ __forceinline__ void enc_store_span(uint8_t* out, int64_t s, int64_t e, int lane, Whole whole, Gen gen) {
  if (s >= e) return;
  const int64_t first = s - (int64_t)((uintptr_t)(out + s) & 15);  // may lie before s (even before 0): only [s, e) is touched
  for (int64_t c = first + (int64_t)lane * 16; c < e; c += 64 * 16) {
    const bool full = c >= s && c + 16 <= e;
    uint64_t v[2] = {0, 0};
    if (full && whole(c, v)) {
    } else {
      const int k0 = c < s ? (int)(s - c) : 0, k1 = e - c < 16 ? (int)(e - c) : 16;
      for (int k = k0; k < k1; ++k) v[k >> 3] |= (uint64_t)gen(c + k) << ((k & 7) * 8);
      if (!full) {  // the ragged ends of the span: its neighbours own the rest of these sixteen bytes
        for (int k = k0; k < k1; ++k) out[c + k] = (uint8_t)(v[k >> 3] >> ((k & 7) * 8));
        continue;
      }
    }
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    u64x2 q;
    q.x = v[0], q.y = v[1];
    *reinterpret_cast<u64x2*>(out + c) = q;
  }
}

// Chosen and Nack: a head of at most ENC_HEAD bytes per record, emitted by the record's lane into LDS, and (Chosen) the
// value's bytes behind it
template <int KIND>
__global__ void __launch_bounds__(ENC_BLOCK) k_enc_emit_hv(const EncArgs a) {
  __shared__ int64_t off[4][65];
  __shared__ int64_t vsrc[4][64];
  __shared__ int64_t wtot[2][4];
  __shared__ uint8_t head[4][64][ENC_HEAD];
  __shared__ uint8_t hlen[4][64];
  if (a.scratch[ENC_W_GO] == 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x;
  const EncHv r = enc_hv<KIND>(a, i);
  int hl = 0;
  if (r.emitted) {
    uint8_t* h = head[wave][lane];
    if (KIND == ENC_NACK) {
      hl = (int)fpxw::nack_emit(h, a.dialect, r.slot);
    } else {
      hl = (int)fpxw::chosen_emit(h, r.slot, nullptr, r.vlen);
      if (r.is_noop) h[hl] = 0x12, h[hl + 1] = 0x00, hl += 2;  // CommandBatchOrNoop{noop}: fpx_wire_emit.hpp NOOP_VALUE
    }
  }
  hlen[wave][lane] = (uint8_t)hl;
  vsrc[wave][lane] = r.voff;
  const int64_t ib = enc_wave_incl_sum(r.bytes), ic = enc_wave_incl_sum((int64_t)r.emitted);
  if (lane == 63) wtot[0][wave] = ib, wtot[1][wave] = ic;
  __syncthreads();
  int64_t at = a.scratch[ENC_W_SUMS + blockIdx.x], midx = a.scratch[ENC_W_SUMS + (size_t)a.nblk + blockIdx.x];
  for (int w = 0; w < wave; ++w) at += wtot[0][w], midx += wtot[1][w];
  at += ib - r.bytes, midx += ic - r.emitted;
  off[wave][lane] = at;
  if (lane == 63) off[wave][64] = at + r.bytes;
  if (r.emitted) a.out_offsets[midx] = at;
  __syncthreads();
  const int64_t* o = off[wave];
  const uint8_t* values = a.values;
  enc_store_span(
      a.out, o[0], o[64], lane,
      [&](int64_t c, uint64_t* v) {
        if (KIND == ENC_NACK) return false;
        const int rec = enc_find(o, c);
        const int64_t q = c - o[rec] - hlen[wave][rec];
        if (q < 0 || c + 16 > o[rec + 1]) return false;  // (a Noop's and a Nack's bytes all lie in the head)
        __builtin_memcpy(v, values + vsrc[wave][rec] + q, 16);  // the piece lies inside one value
        return true;
      },
      [&](int64_t pos) -> uint8_t {
        const int rec = enc_find(o, pos);
        const int64_t q = pos - o[rec];
        if (q < hlen[wave][rec]) return head[wave][rec][q];
        return values[vsrc[wave][rec] + (q - hlen[wave][rec])];
      });
}

// Phase2b: a record is up to 256 generated messages; a lane generates the message a byte belongs to into its own LDS slot
__global__ void __launch_bounds__(ENC_BLOCK) k_enc_emit_p2b(const EncArgs a) {
  __shared__ int64_t off[4][65];
  __shared__ int64_t cnt[4][65];
  __shared__ int64_t wtot[2][4];
  __shared__ uint8_t msg[4][64][ENC_MSG];
  if (a.scratch[ENC_W_GO] == 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t i0 = blockIdx.x * ENC_BLOCK + wave * 64;
  const EncP2b mine = enc_p2b(a, i0 + lane);
  const int64_t bytes = mine.bytes(), count = mine.count();
  const int64_t ib = enc_wave_incl_sum(bytes), ic = enc_wave_incl_sum(count);
  if (lane == 63) wtot[0][wave] = ib, wtot[1][wave] = ic;
  __syncthreads();
  int64_t at = a.scratch[ENC_W_SUMS + blockIdx.x], midx = a.scratch[ENC_W_SUMS + (size_t)a.nblk + blockIdx.x];
  for (int w = 0; w < wave; ++w) at += wtot[0][w], midx += wtot[1][w];
  at += ib - bytes, midx += ic - count;
  off[wave][lane] = at, cnt[wave][lane] = midx;
  if (lane == 63) off[wave][64] = at + bytes, cnt[wave][64] = midx + count;
  __syncthreads();
  const int64_t* o = off[wave];
  const int64_t* m = cnt[wave];
  // the offsets of the wavefront's messages, 64 neighbours at a time
  for (int64_t k = m[0] + lane; k < m[64]; k += 64) {
    const int rec = enc_find(m, k);
    a.out_offsets[k] = o[rec] + enc_p2b(a, i0 + rec).offset_of((int32_t)(k - m[rec]));
  }
  int64_t have_lo = 0, have_hi = 0;  // the message in this lane's slot covers [have_lo, have_hi)
  uint8_t* slot = msg[wave][lane];
  enc_store_span(
      a.out, o[0], o[64], lane, [](int64_t, uint64_t*) { return false; },
      [&](int64_t pos) -> uint8_t {
        if (pos < have_lo || pos >= have_hi) {
          const int rec = enc_find(o, pos);
          const EncP2b r = enc_p2b(a, i0 + rec);
          int32_t j, start, mlen, g, ac;
          r.at((int32_t)(pos - o[rec]), &j, &start, &mlen);
          r.fields(r.select(j), &g, &ac);
          fpxw::phase2b_emit(slot, a.dialect, g, ac, r.slot, r.round);
          have_lo = o[rec] + start, have_hi = have_lo + mlen;
        }
        return slot[pos - have_lo];
      });
}

}  // namespace fpx
