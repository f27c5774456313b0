// fpx_scan.hpp -- the workgroup building blocks of the burst kernels (fpx_*_msgs.hpp, fpx_*_inbox.hpp, fpx_burst_sort.hpp)
// and of the EPaxos kernels (fpx_epaxos.hip and its headers): a wavefront scan, a workgroup scan and reduction, the
// one-workgroup scan of an array in global memory, and a flagged thread's rank.  Templates over the operation (ScanSum,
// ScanMax) and the value type: any 4- or 8-byte integer for ScanSum (an unsigned sum wraps), a signed one for ScanMax.
//
// LDS: the CALLER declares the scratch and passes it in; nothing here declares a __shared__ of its own (one declared in
// an inlined helper would be ONE variable for all the helper's call sites of a kernel).  Every function that takes a
// scratch says how many words it needs, has a barrier between its writes and its reads of them, and leaves it to the
// caller to put a barrier before the same words are used again -- or to pass other words.
//
// Every thread of the workgroup calls these (they shuffle and they meet at barriers); THREADS is the workgroup's size, a
// multiple of 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace fpx {

struct ScanSum {
  template <typename T>
  static __device__ __forceinline__ T identity() { return (T)0; }
  template <typename T>
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
// the maximum of claim words, rounds + 1 and slots + 1: nothing scanned is below -1, which so serves as "nothing yet".
// Signed types only: (T)-1 is the LARGEST value of an unsigned T
struct ScanMax {
  template <typename T>
  static __device__ __forceinline__ T identity() {
    static_assert(std::is_signed<T>::value, "ScanMax scans signed integers: -1 is its 'nothing yet'");
    return (T)-1;
  }
  template <typename T>
  static __device__ __forceinline__ T op(T a, T b) {
    static_assert(std::is_signed<T>::value, "ScanMax scans signed integers: -1 is its 'nothing yet'");
    return b > a ? b : a;
  }
};

// __shfl_up / __shfl_xor of a 4- or 8-byte integer of any name
template <typename T>
__device__ __forceinline__ T scan_shfl_up(T v, int d) {
  if constexpr (sizeof(T) == 4) return (T)__shfl_up((int)v, d);
  else return (T)__shfl_up((long long)v, d);
}
template <typename T>
__device__ __forceinline__ T scan_shfl_xor(T v, int k) {
  if constexpr (sizeof(T) == 4) return (T)__shfl_xor((int)v, k);
  else return (T)__shfl_xor((long long)v, k);
}

// the wavefront's inclusive scan: op over the values of lanes 0 .. this one
template <typename Op, typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = scan_shfl_up(v, d);
    if (lane >= d) v = Op::op(v, o);
  }
  return v;
}

// the workgroup's exclusive scan: op over `carry` and the values of the threads before this one; *total (where asked):
// op over every thread's value, without the carry.  wtot: THREADS / 64 words
template <typename Op, int THREADS, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T carry, T* wtot, T* total = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_incl_scan<Op>(v);
  T excl = scan_shfl_up(inc, 1);  // the wavefront's earlier lanes
  if (lane == 0) excl = Op::template identity<T>();
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  T before = carry;
  for (int w = 0; w < wave; ++w) before = Op::op(before, wtot[w]);
  if (total) {
    T all = wtot[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) all = Op::op(all, wtot[w]);
    *total = all;
  }
  return Op::op(before, excl);
}

// op over the values of the wavefront's 64 lanes, in every lane
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    v = Op::op(v, scan_shfl_xor(v, k));
  }
  return v;
}

// op over every thread's value, in every thread.  w: THREADS / 64 words; ends with a barrier, so `w` is free again
template <typename Op, int THREADS, typename T>
__device__ __forceinline__ T block_reduce(T v, T* w) {
  v = wave_reduce<Op>(v);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = w[0];
#pragma unroll
  for (int j = 1; j < THREADS / 64; ++j) r = Op::op(r, w[j]);
  __syncthreads();
  return r;
}

// ONE workgroup rewrites a[0 .. len) in place to its exclusive scan, THREADS * PER elements a step (a thread takes PER
// consecutive ones) with a carry from step to step that begins as `start`, and returns op over `start` and all of a --
// `start` when len is 0 -- to every thread.  len and start may come from device memory; every thread passes the same.
// lds: SCAN_ARRAY_LDS(THREADS) words
#define SCAN_ARRAY_LDS(THREADS) ((THREADS) / 64 + 1)
template <typename Op, int THREADS, int PER, typename T, typename Len>
__device__ __forceinline__ T scan_array_excl(T* a, Len len, T* lds, T start = Op::template identity<T>()) {
  T* carry = lds + THREADS / 64;
  const int t = threadIdx.x;
  if (t == 0) *carry = start;
  __syncthreads();
  for (Len base = 0; base < len; base += THREADS * PER) {
    const Len b0 = base + (Len)t * PER;
    T v[PER], mine = Op::template identity<T>();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      v[j] = b0 + j < len ? a[b0 + j] : Op::template identity<T>();
      mine = Op::op(mine, v[j]);
    }
    const T before = block_excl_scan<Op, THREADS>(mine, *carry, lds);
    T at = before;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (b0 + j < len) a[b0 + j] = at;
      at = Op::op(at, v[j]);
    }
    __syncthreads();
    if (t == THREADS - 1) *carry = Op::op(before, mine);
    __syncthreads();
  }
  return *carry;
}

// this thread's rank among the workgroup's flagged threads, and the workgroup's count (256 threads).  wsum: 4 words
__device__ __forceinline__ int block_rank(bool flag, int* total, int* wsum) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  *total = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace fpx
