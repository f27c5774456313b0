// fpx_epaxos_rec.hpp -- the record of K5's second form (fpx_epaxos_kp.hpp): one command as k_kp_scatter writes it into its
// key's segment and k_epx_key2 reads it back.  A header of its own so that tests/epaxos_record_harness.hip can pack and
// unpack records directly (tests/test_gpu_epaxos_record.py).  Included inside a namespace, after <hip/hip_runtime.h> and
// <cstdint>; it includes nothing itself.
#pragma once

constexpr int KP_IDX_BITS = 21;          // message indices and ranks: m < 2^21
constexpr uint32_t KP_IDX_MASK = (1u << KP_IDX_BITS) - 1u;

// flags of a command as the key kernel keeps them: leader | is_set << 3 | resp_mask << 8 | seen_mask << 16
__device__ __forceinline__ int kp_flags(int L, int is_set, unsigned resp, unsigned seen) {
  return L | (is_set ? 8 : 0) | (int)(resp << 8) | (int)(seen << 16);
}

// The record.  resp_mask is n - 2 of the n - 1 replicas that are not the leader: the header names the ONE that is left
// out (its index among the non-leaders), which with leader, is_set and seen_mask fits beside a 21-bit message index for
// n <= 5.  Ranks are < m < 2^21: two ranks' words carry a third rank's halves in their upper 11 bits.
template <int N>
__device__ __forceinline__ void kp_pack(uint32_t* w, int i, int x, int L, int is_set, unsigned resp, unsigned seen, const int* rk) {
  const unsigned full = (1u << N) - 1u;
  const int q = __ffs((int)(full & ~resp & ~(1u << L))) - 1;  // the non-leader whose answer is not waited for
  const unsigned e = (unsigned)(q - (q > L ? 1 : 0));
  const unsigned hdr = (unsigned)L | (is_set ? 8u : 0u) | (seen << 4) | (e << (4 + N));
  auto pair_lo = [](int a, int c) { return (uint32_t)a | (((uint32_t)c & 0x7ffu) << KP_IDX_BITS); };
  auto pair_hi = [](int a, int c) { return (uint32_t)a | (((uint32_t)c >> 11) << KP_IDX_BITS); };
  if constexpr (N <= 3) {
    w[0] = (uint32_t)i | (hdr << KP_IDX_BITS), w[1] = (uint32_t)x;
    w[2] = pair_lo(rk[0], rk[2]), w[3] = pair_hi(rk[1], rk[2]);
  } else if constexpr (N <= 5) {
    w[0] = (uint32_t)i | (hdr << KP_IDX_BITS), w[1] = (uint32_t)x;
    w[2] = pair_lo(rk[0], rk[4]), w[3] = pair_hi(rk[1], rk[4]), w[4] = (uint32_t)rk[2], w[5] = (uint32_t)rk[3];
  } else {
    w[0] = (uint32_t)i, w[1] = (uint32_t)x, w[2] = (uint32_t)kp_flags(L, is_set, resp, seen);
    w[3] = pair_lo(rk[0], rk[4]), w[4] = pair_hi(rk[1], rk[4]);
    w[5] = pair_lo(rk[2], rk[5]), w[6] = pair_hi(rk[3], rk[5]), w[7] = (uint32_t)rk[6];
  }
}

template <int N>
__device__ __forceinline__ void kp_unpack(const uint32_t* w, int* i, int* x, int* flags, int* rk) {
  auto third = [](uint32_t a, uint32_t c) { return (int)((a >> KP_IDX_BITS) | ((c >> KP_IDX_BITS) << 11)); };
  if constexpr (N <= 5) {
    *i = (int)(w[0] & KP_IDX_MASK), *x = (int)w[1];
    const unsigned hdr = w[0] >> KP_IDX_BITS, full = (1u << N) - 1u;
    const int L = (int)(hdr & 7u);
    const unsigned seen = (hdr >> 4) & full, e = hdr >> (4 + N);
    const unsigned q = e + (e >= (unsigned)L ? 1u : 0u);
    *flags = kp_flags(L, (int)((hdr >> 3) & 1u), full & ~(1u << L) & ~(1u << q), seen);
    rk[0] = (int)(w[2] & KP_IDX_MASK), rk[1] = (int)(w[3] & KP_IDX_MASK);
    if constexpr (N <= 3) {
      rk[2] = third(w[2], w[3]);
    } else {
      rk[2] = (int)w[4], rk[3] = (int)w[5], rk[4] = third(w[2], w[3]);
    }
  } else {
    *i = (int)w[0], *x = (int)w[1], *flags = (int)w[2];
    rk[0] = (int)(w[3] & KP_IDX_MASK), rk[1] = (int)(w[4] & KP_IDX_MASK), rk[4] = third(w[3], w[4]);
    rk[2] = (int)(w[5] & KP_IDX_MASK), rk[3] = (int)(w[6] & KP_IDX_MASK), rk[5] = third(w[5], w[6]);
    rk[6] = (int)w[7];
  }
}
