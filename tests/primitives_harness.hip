// primitives_harness.hip -- test-only launchers for the workgroup primitives of frankenpaxos_amd/csrc/fpx_scan.hpp and the
// radix sort of fpx_burst_sort.hpp, one extern "C" function per instantiation: pt_<primitive>_<op>_<type>_<threads>[_<per>]
// (types: int, u32 = uint32_t, i64 = int64_t, ll = long long).  tests/primitives.py builds this file into
// tests/_build/libfpx_primitives.so, names every launcher in a table, lists the library's call sites with the launcher
// that stands for each (USES) and holds the exact references; tests/test_gpu_primitives.py compares.  Nothing else of the library is included and no library context is used: the
// buffers are the test's device tensors.
//
// A wrapper writes what the primitive returns to out[global thread id] (and a *total to a second array) and never uses a
// result as an address, so a wrong primitive shows as a wrong value.  The one exception is the sort's own scatter, which
// the launcher lets run only on lengths it has checked.  The LDS a primitive gets is declared here at exactly the word
// count the header documents, between GUARD words on either side that the wrapper copies out afterwards: a primitive
// that uses more than it documents changes a guard.
//
// A launcher checks its arguments on the host and returns PT_EARG (or PT_ENULL) without launching when they are off;
// otherwise it launches on the stream it is given, waits for that stream, and returns the HIP error (0: none).
#include "fpx_burst_sort.hpp"
#include "fpx_scan.hpp"

using namespace fpx;

namespace {

constexpr int PT_EARG = -1;      // an argument out of range
constexpr int PT_ENULL = -2;     // a pointer missing (looked at after the ranges)
constexpr int GUARD = 2;         // guard words on either side of a wrapper's scratch
constexpr int ROUNDS = 64;       // of the LDS-reuse wrappers
constexpr int ARRAY_BLOCKS = 16; // arrays (workgroups) a scan_array launch takes at the most
constexpr int ARRAY_PAD = 64;    // words behind an array's capacity that the test checks for its sentinel

template <typename T>
__device__ __forceinline__ T guard_word() {
  return (T)0x5a5a5a5a5a5a5a5aull;
}

// WORDS words of scratch for a primitive, fenced
template <typename T, int WORDS>
struct Guarded {
  T lo[GUARD];
  T w[WORDS];
  T hi[GUARD];
};

template <typename T, int WORDS>
__device__ __forceinline__ void guard_arm(Guarded<T, WORDS>& s) {
  if (threadIdx.x < GUARD) s.lo[threadIdx.x] = guard_word<T>(), s.hi[threadIdx.x] = guard_word<T>();
  __syncthreads();
}
// guards: [blocks][2 * GUARD]
template <typename T, int WORDS>
__device__ __forceinline__ void guard_read(Guarded<T, WORDS>& s, T* guards) {
  __syncthreads();
  if (threadIdx.x < GUARD) {
    guards[blockIdx.x * 2 * GUARD + threadIdx.x] = s.lo[threadIdx.x];
    guards[blockIdx.x * 2 * GUARD + GUARD + threadIdx.x] = s.hi[threadIdx.x];
  }
}

template <typename K, typename... A>
int launch(K kernel, int blocks, int threads, void* stream, A... args) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, args...);
  const hipError_t waited = hipStreamSynchronize(s);
  const hipError_t last = hipGetLastError();
  return (int)(last != hipSuccess ? last : waited);
}

// ---- the wavefront functions: no LDS ----
template <typename Op, typename T>
__global__ void k_wave_incl_scan(const T* in, T* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  out[g] = wave_incl_scan<Op>(in[g]);
}
template <typename Op, typename T>
__global__ void k_wave_reduce(const T* in, T* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  out[g] = wave_reduce<Op>(in[g]);
}

// ---- the workgroup functions: a workgroup's own values, its own carry ----
// total_out[g]: the *total this thread was given, or the guard word where the call asks for none
template <typename Op, int THREADS, typename T, bool TOTAL>
__global__ void __launch_bounds__(THREADS) k_block_excl_scan(const T* in, const T* carry, T* out, T* total_out, T* guards) {
  __shared__ Guarded<T, THREADS / 64> s;
  guard_arm(s);
  const int g = blockIdx.x * THREADS + threadIdx.x;
  T total = guard_word<T>();
  if constexpr (TOTAL) out[g] = block_excl_scan<Op, THREADS>(in[g], carry[blockIdx.x], s.w, &total);
  else out[g] = block_excl_scan<Op, THREADS>(in[g], carry[blockIdx.x], s.w);
  total_out[g] = total;
  guard_read(s, guards);
}

template <typename Op, int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) k_block_reduce(const T* in, T* out, T* guards) {
  __shared__ Guarded<T, THREADS / 64> s;
  guard_arm(s);
  const int g = blockIdx.x * THREADS + threadIdx.x;
  out[g] = block_reduce<Op, THREADS>(in[g], s.w);
  guard_read(s, guards);
}

__global__ void __launch_bounds__(256) k_block_rank(const uint8_t* flag, int* out, int* total_out, int* guards) {
  __shared__ Guarded<int, 4> s;
  guard_arm(s);
  const int g = blockIdx.x * 256 + threadIdx.x;
  int total = guard_word<int>();
  out[g] = block_rank(flag[g] != 0, &total, s.w);
  total_out[g] = total;
  guard_read(s, guards);
}

// ---- scan_array_excl: workgroup b scans a[b * stride .. + len[b]) ----
struct ArrayArgs {
  long long len[ARRAY_BLOCKS], start[ARRAY_BLOCKS];
};
template <typename Op, int THREADS, int PER, typename T, typename Len, bool START>
__global__ void __launch_bounds__(THREADS) k_scan_array_excl(T* a, long long stride, const ArrayArgs g, T* out, T* guards) {
  __shared__ Guarded<T, SCAN_ARRAY_LDS(THREADS)> s;
  guard_arm(s);
  T* mine = a + blockIdx.x * stride;
  const Len len = (Len)g.len[blockIdx.x];
  T all;
  if constexpr (START) all = scan_array_excl<Op, THREADS, PER>(mine, len, s.w, (T)g.start[blockIdx.x]);
  else all = scan_array_excl<Op, THREADS, PER>(mine, len, s.w);
  out[blockIdx.x * THREADS + threadIdx.x] = all;
  guard_read(s, guards);
}

// ---- the LDS-reuse contract: ROUNDS rounds on the same words, in/out [ROUNDS][2][blocks * THREADS] ----
// block_reduce twice in a row on the same words: it ends with a barrier
template <typename Op, int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) k_reduce_twice(const T* in, T* out, T* guards) {
  __shared__ Guarded<T, THREADS / 64> s;
  guard_arm(s);
  const size_t n = (size_t)gridDim.x * THREADS, g = (size_t)blockIdx.x * THREADS + threadIdx.x;
  for (int r = 0; r < ROUNDS; ++r) {
    const T a = block_reduce<Op, THREADS>(in[(2 * r) * n + g], s.w);
    const T b = block_reduce<Op, THREADS>(in[(2 * r + 1) * n + g], s.w);
    out[(2 * r) * n + g] = a, out[(2 * r + 1) * n + g] = b;
  }
  guard_read(s, guards);
}
// block_excl_scan twice on the same words, the caller's barrier after each (k_dg_emit, k_ri_execby); the first call's
// total is the second's carry.  total_out as out
template <typename Op, int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) k_scan_twice_same_words(const T* in, T* out, T* total_out, T* guards) {
  __shared__ Guarded<T, THREADS / 64> s;
  guard_arm(s);
  const size_t n = (size_t)gridDim.x * THREADS, g = (size_t)blockIdx.x * THREADS + threadIdx.x;
  for (int r = 0; r < ROUNDS; ++r) {
    T ta, tb;
    const T a = block_excl_scan<Op, THREADS>(in[(2 * r) * n + g], Op::template identity<T>(), s.w, &ta);
    __syncthreads();
    const T b = block_excl_scan<Op, THREADS>(in[(2 * r + 1) * n + g], ta, s.w, &tb);
    __syncthreads();
    out[(2 * r) * n + g] = a, out[(2 * r + 1) * n + g] = b;
    total_out[(2 * r) * n + g] = ta, total_out[(2 * r + 1) * n + g] = tb;
  }
  guard_read(s, guards);
}
// block_excl_scan twice on different words with no barrier between (the digit starts of k_rs_scatter); one barrier a round
template <typename Op, int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) k_scan_twice_other_words(const T* in, T* out, T* guards) {
  __shared__ Guarded<T, 2 * (THREADS / 64)> s;
  guard_arm(s);
  const size_t n = (size_t)gridDim.x * THREADS, g = (size_t)blockIdx.x * THREADS + threadIdx.x;
  for (int r = 0; r < ROUNDS; ++r) {
    const T a = block_excl_scan<Op, THREADS>(in[(2 * r) * n + g], Op::template identity<T>(), s.w);
    const T b = block_excl_scan<Op, THREADS>(in[(2 * r + 1) * n + g], Op::template identity<T>(), s.w + THREADS / 64);
    out[(2 * r) * n + g] = a, out[(2 * r + 1) * n + g] = b;
    __syncthreads();
  }
  guard_read(s, guards);
}

template <typename Op, int THREADS, int PER, typename T, typename Len, bool START>
int launch_scan_array(void* stream, void* a, long long capacity, const long long* len, const long long* start, int blocks,
                      void* out, void* guards) {
  if (blocks < 1 || blocks > ARRAY_BLOCKS || capacity < 0 || !len || (START && !start)) return PT_EARG;
  ArrayArgs g = {};
  for (int b = 0; b < blocks; ++b) {
    if (len[b] < 0 || len[b] > capacity) return PT_EARG;
    g.len[b] = len[b], g.start[b] = START ? start[b] : 0;
  }
  return launch(k_scan_array_excl<Op, THREADS, PER, T, Len, START>, blocks, THREADS, stream, (T*)a,
                capacity + ARRAY_PAD, g, (T*)out, (T*)guards);
}

// the scratch of a sort of `tiles` tiles, cut the way the library cuts it
SortScratch carve_sort(void* base, int tiles, size_t* bytes) {
  Carver c(base);
  const SortScratch s = lay_sort(c, (size_t)tiles);
  *bytes = c.size();
  return s;
}

}  // namespace

typedef long long ll;
typedef uint32_t u32;
typedef int64_t i64;

#define PT_WAVE(FN, OPNAME, OP, T, THREADS)                                                          \
  extern "C" int pt_##FN##_##OPNAME##_##T##_##THREADS(void* stream, const void* in, void* out, int blocks) { \
    if (blocks < 1) return PT_EARG;                                                                  \
    return launch(k_##FN<OP, T>, blocks, THREADS, stream, (const T*)in, (T*)out);                    \
  }
#define PT_WAVE_BOTH(OPNAME, OP, T)           \
  PT_WAVE(wave_incl_scan, OPNAME, OP, T, 64)  \
  PT_WAVE(wave_incl_scan, OPNAME, OP, T, 256) \
  PT_WAVE(wave_reduce, OPNAME, OP, T, 64)     \
  PT_WAVE(wave_reduce, OPNAME, OP, T, 256)
PT_WAVE_BOTH(sum, ScanSum, int)
PT_WAVE_BOTH(sum, ScanSum, u32)
PT_WAVE_BOTH(sum, ScanSum, i64)
PT_WAVE_BOTH(sum, ScanSum, ll)
PT_WAVE_BOTH(max, ScanMax, int)
PT_WAVE_BOTH(max, ScanMax, i64)
PT_WAVE_BOTH(max, ScanMax, ll)

// in, out, total_out: [blocks * THREADS]; carry: [blocks]; guards: [blocks][2 * GUARD]
#define PT_BLOCK_EXCL_SCAN(OPNAME, OP, T, THREADS, SUFFIX, TOTAL)                                                     \
  extern "C" int pt_block_excl_scan_##OPNAME##_##T##_##THREADS##SUFFIX(void* stream, const void* in, const void* carry, \
                                                                       void* out, void* total_out, void* guards,      \
                                                                       int blocks) {                                  \
    if (blocks < 1) return PT_EARG;                                                                                   \
    return launch(k_block_excl_scan<OP, THREADS, T, TOTAL>, blocks, THREADS, stream, (const T*)in, (const T*)carry,   \
                  (T*)out, (T*)total_out, (T*)guards);                                                                \
  }
PT_BLOCK_EXCL_SCAN(sum, ScanSum, u32, 256, , false)
PT_BLOCK_EXCL_SCAN(sum, ScanSum, u32, 256, _total, true)
PT_BLOCK_EXCL_SCAN(sum, ScanSum, u32, 512, , false)
PT_BLOCK_EXCL_SCAN(sum, ScanSum, i64, 1024, _total, true)
PT_BLOCK_EXCL_SCAN(max, ScanMax, int, 256, , false)
PT_BLOCK_EXCL_SCAN(max, ScanMax, ll, 256, , false)

#define PT_BLOCK_REDUCE(OPNAME, OP, T, THREADS)                                                                        \
  extern "C" int pt_block_reduce_##OPNAME##_##T##_##THREADS(void* stream, const void* in, void* out, void* guards,     \
                                                            int blocks) {                                              \
    if (blocks < 1) return PT_EARG;                                                                                    \
    return launch(k_block_reduce<OP, THREADS, T>, blocks, THREADS, stream, (const T*)in, (T*)out, (T*)guards);         \
  }
PT_BLOCK_REDUCE(sum, ScanSum, u32, 256)
PT_BLOCK_REDUCE(sum, ScanSum, int, 256)
PT_BLOCK_REDUCE(max, ScanMax, int, 256)
PT_BLOCK_REDUCE(max, ScanMax, ll, 256)
PT_BLOCK_REDUCE(max, ScanMax, int, 1024)
PT_BLOCK_REDUCE(max, ScanMax, i64, 1024)  // (no caller: the 8-byte reduction over sixteen wavefronts)

extern "C" int pt_block_rank_256(void* stream, const void* flag, void* out, void* total_out, void* guards, int blocks) {
  if (blocks < 1) return PT_EARG;
  return launch(k_block_rank, blocks, 256, stream, (const uint8_t*)flag, (int*)out, (int*)total_out, (int*)guards);
}

// a: [blocks][capacity + ARRAY_PAD]; len, start: HOST arrays of `blocks` (start: null without _start); out: [blocks * THREADS]
#define PT_SCAN_ARRAY(OPNAME, OP, T, THREADS, PER, LEN)                                                                \
  extern "C" int pt_scan_array_excl_##OPNAME##_##T##_##THREADS##_##PER(void* stream, void* a, long long capacity,      \
                                                                       const long long* len, int blocks, void* out,    \
                                                                       void* guards) {                                 \
    return launch_scan_array<OP, THREADS, PER, T, LEN, false>(stream, a, capacity, len, nullptr, blocks, out, guards); \
  }                                                                                                                    \
  extern "C" int pt_scan_array_excl_##OPNAME##_##T##_##THREADS##_##PER##_start(                                        \
      void* stream, void* a, long long capacity, const long long* len, const long long* start, int blocks, void* out,  \
      void* guards) {                                                                                                  \
    return launch_scan_array<OP, THREADS, PER, T, LEN, true>(stream, a, capacity, len, start, blocks, out, guards);    \
  }
PT_SCAN_ARRAY(sum, ScanSum, u32, 256, 1, int)
PT_SCAN_ARRAY(sum, ScanSum, int, 1024, 1, int)
PT_SCAN_ARRAY(sum, ScanSum, int, 1024, 8, ll)
PT_SCAN_ARRAY(max, ScanMax, int, 256, 1, int)
PT_SCAN_ARRAY(max, ScanMax, int, 1024, 1, int)
PT_SCAN_ARRAY(max, ScanMax, ll, 1024, 1, int)

// in, out (and total_out): [ROUNDS][2][blocks * THREADS]
extern "C" int pt_reduce_twice_sum_u32_256(void* stream, const void* in, void* out, void* guards, int blocks) {
  if (blocks < 1) return PT_EARG;
  return launch(k_reduce_twice<ScanSum, 256, u32>, blocks, 256, stream, (const u32*)in, (u32*)out, (u32*)guards);
}
extern "C" int pt_reduce_twice_sum_int_256(void* stream, const void* in, void* out, void* guards, int blocks) {  // k_mk_total
  if (blocks < 1) return PT_EARG;
  return launch(k_reduce_twice<ScanSum, 256, int>, blocks, 256, stream, (const int*)in, (int*)out, (int*)guards);
}
extern "C" int pt_reduce_twice_max_ll_256(void* stream, const void* in, void* out, void* guards, int blocks) {
  if (blocks < 1) return PT_EARG;
  return launch(k_reduce_twice<ScanMax, 256, ll>, blocks, 256, stream, (const ll*)in, (ll*)out, (ll*)guards);
}
extern "C" int pt_scan_twice_same_words_sum_u32_256(void* stream, const void* in, void* out, void* total_out, void* guards,
                                                    int blocks) {
  if (blocks < 1) return PT_EARG;
  return launch(k_scan_twice_same_words<ScanSum, 256, u32>, blocks, 256, stream, (const u32*)in, (u32*)out, (u32*)total_out,
                (u32*)guards);
}
extern "C" int pt_scan_twice_other_words_sum_u32_512(void* stream, const void* in, void* out, void* guards, int blocks) {
  if (blocks < 1) return PT_EARG;
  return launch(k_scan_twice_other_words<ScanSum, 512, u32>, blocks, 512, stream, (const u32*)in, (u32*)out, (u32*)guards);
}

extern "C" int pt_rounds() { return ROUNDS; }
extern "C" int pt_guard_words() { return GUARD; }
extern "C" int pt_array_pad() { return ARRAY_PAD; }
extern "C" int pt_array_blocks() { return ARRAY_BLOCKS; }

// ---- the sort ----
extern "C" long long pt_sort_scratch_bytes(int tiles) {
  if (tiles < 1) return PT_EARG;
  size_t bytes;
  (void)carve_sort(nullptr, tiles, &bytes);
  return (long long)bytes;
}
// the byte offsets of hist, key[0], key[1], val[0], val[1] in that scratch
extern "C" int pt_sort_scratch_offsets(int tiles, long long* at) {
  if (tiles < 1 || !at) return PT_EARG;
  const uintptr_t base = (uintptr_t)1 << 30;  // never read or written: only the distances count
  size_t bytes;
  const SortScratch s = carve_sort((void*)base, tiles, &bytes);
  at[0] = (long long)((uintptr_t)s.hist - base);
  for (int j = 0; j < 2; ++j) at[1 + j] = (long long)((uintptr_t)s.key[j] - base), at[3 + j] = (long long)((uintptr_t)s.val[j] - base);
  return 0;
}
// Sorts the `len` pairs the test has put into key[0], val[0] of `scratch` (pt_sort_scratch_bytes(tiles) bytes).  The
// launcher writes `len` to *d_len itself, so the length the kernels read is the one checked here.  *r: what burst_sort
// returned.  val_last: null, or tiles * 256 words
extern "C" int pt_burst_sort(void* stream, void* scratch, long long scratch_bytes, void* d_len, int len, long long max_key,
                             int tiles, void* val_last, int* r) {
  if (tiles < 1 || max_key < 0 || len < 0 || len > (long long)tiles * SORT_TILE) return PT_EARG;
  size_t bytes;
  const SortScratch s = carve_sort(scratch, tiles, &bytes);  // (pointer arithmetic only)
  if ((long long)bytes > scratch_bytes) return PT_EARG;
  if (!scratch || !d_len || !r) return PT_ENULL;
  hipStream_t st = (hipStream_t)stream;
  const int32_t m = len;
  hipError_t e = hipMemcpyAsync(d_len, &m, sizeof m, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  *r = burst_sort(st, (const int32_t*)d_len, s, (int64_t)max_key, tiles, (int32_t*)val_last);
  const hipError_t waited = hipStreamSynchronize(st);
  const hipError_t last = hipGetLastError();
  return (int)(last != hipSuccess ? last : waited);
}
