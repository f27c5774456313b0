// fpx_burst_sort.hpp -- the stable LSD radix sort of the burst calls: (key, value) pairs of int32, SORT_RADIX_BITS bits per
// pass, tile <-> workgroup, in the shape of k_rs_hist / k_rs_scan / k_rs_scatter of fpx_epaxos.hip.  The number of pairs
// is a word in device memory (the replica inbox sorts its reads, and how many there are is known only there).
//
//   k_sort_count    workgroup / tile: the tile's count of every digit, digit-major
//   k_sort_scan     one workgroup: the exclusive sums of those counts, SORT_SCAN_PER consecutive counts per thread and step
//                   (the counts are SORT_RADIX per 256 pairs -- 131 072 words at 2^21 pairs -- and one workgroup that takes
//                   one count per thread and step spends longer on them than any other pass: profiles/acceptor_inbox.md)
//   k_sort_scatter  workgroup / tile: a pair's place among the equal digits of its tile is its rank by position (ballots),
//                   never a cursor handed out by an atomic
//
// burst_sort() launches the passes.
#pragma once
#include "fpx_scan.hpp"
#include "fpx_scratch.hpp"

namespace fpx {

constexpr int SORT_TILE = BURST_TILE;  // pairs per tile (one per thread)
constexpr int SORT_SCAN_PER = 8;

struct BurstSort {
  const int32_t* len;  // the number of pairs
  int32_t* hist;       // [SORT_RADIX][tiles]
  const int32_t *key_in, *val_in;
  int32_t *key_out, *val_out;
  int shift;
};

__global__ void __launch_bounds__(256) k_sort_count(const BurstSort a) {
  __shared__ int wc[4][SORT_RADIX];
  const int m = *a.len, tiles = (m + SORT_TILE - 1) / SORT_TILE, tile = blockIdx.x;
  if (tile >= tiles) return;
  const int j = tile * SORT_TILE + threadIdx.x;
  const int d = j < m ? (a.key_in[j] >> a.shift) & (SORT_RADIX - 1) : -1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < SORT_RADIX; ++v) {
    const int c = __popcll(__ballot(d == v));
    if (lane == 0) wc[wave][v] = c;
  }
  __syncthreads();
  if (threadIdx.x < SORT_RADIX) {
    const int v = threadIdx.x;
    a.hist[(size_t)v * tiles + tile] = wc[0][v] + wc[1][v] + wc[2][v] + wc[3][v];
  }
}

__global__ void __launch_bounds__(1024) k_sort_scan(const BurstSort a) {
  __shared__ int lds[SCAN_ARRAY_LDS(1024)];
  const int m = *a.len, tiles = (m + SORT_TILE - 1) / SORT_TILE;
  (void)scan_array_excl<ScanSum, 1024, SORT_SCAN_PER>(a.hist, (long long)tiles * SORT_RADIX, lds);
}

__global__ void __launch_bounds__(256) k_sort_scatter(const BurstSort a) {
  __shared__ int wc[4][SORT_RADIX];
  const int m = *a.len, tiles = (m + SORT_TILE - 1) / SORT_TILE, tile = blockIdx.x;
  if (tile >= tiles) return;
  const int j = tile * SORT_TILE + threadIdx.x;
  const bool valid = j < m;
  const int key = valid ? a.key_in[j] : 0, val = valid ? a.val_in[j] : 0;
  const int d = (key >> a.shift) & (SORT_RADIX - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 4 * SORT_RADIX) (&wc[0][0])[threadIdx.x] = 0;
  __syncthreads();
  // the lanes of this wavefront with the same digit
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < SORT_RADIX_BITS; ++bit) {
    const bool one = (d >> bit) & 1;
    const unsigned long long mk = __ballot(valid && one);
    peers &= one ? mk : ~mk;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (valid && rank == 0) wc[wave][d] = __popcll(peers);
  __syncthreads();
  if (!valid) return;
  int at = a.hist[(size_t)d * tiles + tile] + rank;
  for (int w = 0; w < wave; ++w) at += wc[w][d];
  a.key_out[at] = key, a.val_out[at] = val;
}

// Sorts the *d_len pairs (s.key[0], s.val[0]) by keys 0 .. max_key; `tiles` is the grid: the tiles *d_len can come to.
// The sorted keys end up in s.key[r] and the values in s.val[r] for the r returned -- or in val_last, where given.  There
// is always at least one pass, so that holds for max_key == 0 (every key 0) too: r is then 1
inline int burst_sort(hipStream_t stream, const int32_t* d_len, const SortScratch& s, int64_t max_key, int tiles,
                      int32_t* val_last = nullptr) {
  int bits = 0;
  while (max_key >> bits) ++bits;
  const int passes = bits ? (bits + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS : 1;
  const dim3 per_tile(tiles), blk(256);
  for (int p = 0; p < passes; ++p) {
    BurstSort a;
    a.len = d_len, a.hist = s.hist, a.shift = p * SORT_RADIX_BITS;
    a.key_in = s.key[p & 1], a.val_in = s.val[p & 1];
    a.key_out = s.key[(p + 1) & 1], a.val_out = p + 1 == passes && val_last ? val_last : s.val[(p + 1) & 1];
    hipLaunchKernelGGL(k_sort_count, per_tile, blk, 0, stream, a);
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(1024), 0, stream, a);
    hipLaunchKernelGGL(k_sort_scatter, per_tile, blk, 0, stream, a);
  }
  return passes & 1;
}

}  // namespace fpx
