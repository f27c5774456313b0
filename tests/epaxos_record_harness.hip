// Test-only harness of the record of K5's second form (frankenpaxos_amd/csrc/fpx_epaxos_rec.hpp): one kernel per n that
// packs arrays of commands into records with kp_pack and unpacks them again with kp_unpack, exactly the two functions
// k_kp_scatter and k_epx_key2 call.  tests/epaxos_record.py builds it into tests/_build and
// tests/test_gpu_epaxos_record.py checks the round trip.  Not part of libfpx.so.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {
#include "fpx_epaxos_rec.hpp"

template <int N> struct Rec { static constexpr int NI = N <= 3 ? 4 : N <= 5 ? 6 : 8; };  // words of a record (KpTile<N>::NI)

// command c: index i[c], number x[c], leader L[c], is_set[c], resp[c], seen[c], ranks rk[q * count + c]
template <int N>
__global__ void __launch_bounds__(256) k_record_round_trip(int count, const int* i, const int* x, const int* L, const int* is_set,
                                                           const int* resp, const int* seen, const int* rk, uint32_t* words,
                                                           int* oi, int* ox, int* oflags, int* ork) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  int r[N], back[N];
#pragma unroll
  for (int q = 0; q < N; ++q) r[q] = rk[(size_t)q * count + c];
  uint32_t w[Rec<N>::NI];
  kp_pack<N>(w, i[c], x[c], L[c], is_set[c], (unsigned)resp[c], (unsigned)seen[c], r);
#pragma unroll
  for (int h = 0; h < Rec<N>::NI; ++h) words[(size_t)c * Rec<N>::NI + h] = w[h];
  kp_unpack<N>(w, &oi[c], &ox[c], &oflags[c], back);
#pragma unroll
  for (int q = 0; q < N; ++q) ork[(size_t)q * count + c] = back[q];
}

template <int N>
int round_trip(int count, const int* i, const int* x, const int* L, const int* is_set, const int* resp, const int* seen,
               const int* rk, uint32_t* words, int* oi, int* ox, int* oflags, int* ork) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL((k_record_round_trip<N>), dim3((count + 255) / 256), dim3(256), 0, 0, count, i, x, L, is_set, resp, seen,
                     rk, words, oi, ox, oflags, ork);
  if (hipGetLastError() != hipSuccess) return -1;
  return hipDeviceSynchronize() == hipSuccess ? 0 : -2;
}
}  // namespace

// every pointer is device memory; words has count * er_record_words(n) entries.  Returns 0, or < 0 on a HIP error
extern "C" int er_record_words(int n) { return n <= 3 ? Rec<3>::NI : n <= 5 ? Rec<5>::NI : Rec<7>::NI; }
extern "C" int er_round_trip(int n, int count, const int* i, const int* x, const int* L, const int* is_set, const int* resp,
                             const int* seen, const int* rk, uint32_t* words, int* oi, int* ox, int* oflags, int* ork) {
  switch (n) {
    case 3: return round_trip<3>(count, i, x, L, is_set, resp, seen, rk, words, oi, ox, oflags, ork);
    case 5: return round_trip<5>(count, i, x, L, is_set, resp, seen, rk, words, oi, ox, oflags, ork);
    case 7: return round_trip<7>(count, i, x, L, is_set, resp, seen, rk, words, oi, ox, oflags, ork);
  }
  return -3;
}
