// fpx_epaxos_mk.hpp -- multi-key get / set commands through K5 / K7 (included by fpx_epaxos.hip, inside its namespace).
//
// KeyValueStore.scala:221-302 (typedTopKConflictIndex, k = 1): a command's top-one conflicts are the element-wise max,
// over its keys, of each key's TopOne state (a get conflicts with the sets of its keys, a set with their gets and sets),
// and put records the instance under every key.  Each key's state moves only through commands on that key, so the tick splits into
// (command, distinct key) pairs that run through K5's first form unchanged -- sort by key, segments, k_epx_scan over the
// pairs -- and one max per command over its pairs' rows gives the conf[m][n][NP] rows k_epx_decide consumes:
//   k_mk_prep      one thread per command: offsets monotone, keys in [0, num_keys), the count of DISTINCT keys
//                  (a repeat would be the command's own conflict: see own_column), totals for the host
//   k_mk_pairs     uniq[j] (first occurrence of its key in its command) and the pair's instance number
//   k_mk_place     (tick) every command's record at its position in every replica's delivery order
//   k_mk_tilesum / k_mk_tilescan / k_mk_scatter   one exclusive scan of the distinct-key counts per replica (all n in
//                  one launch each), then the pairs at scan offset + index: the replica's pair sequence in its order
//   k_mk_merge     conf row of (command, replica) = max over the command's pair rows
// A command without keys has no pairs: its rows are zero (no dependencies) and it teaches the index nothing -- as the
// reference's empty merge and empty put.

constexpr int MK_TILE = 1024;  // positions of one scan tile: 256 threads x 4
constexpr uint32_t MK_U_MASK = (1u << EPX_SET_SHIFT) - 1u;

struct MkBatch {
  int m, P, U, tiles;
  const int32_t* off;   // [m + 1]
  const int32_t* keys;  // [P]
  const int32_t* leader;
  const int32_t* number;
  const uint8_t* is_set;
  const uint8_t* resp_mask;
  const uint8_t* seen_mask;
  const int32_t* rank;  // [n][m]
  int32_t* ucnt;        // [m] distinct keys of the command
  int32_t* info;        // [0] sum of ucnt, [1] commands whose list is not exactly one key, [2] key_off[m], [3] status
  int2* part;           // [blocks of k_mk_prep] its partial sums of ucnt and of commands without exactly one key
  uint8_t* uniq;        // [P]
  int32_t* pnum;        // [P] the instance number of the pair's command
  int4* rec;            // [n][m] at the command's position p in replica r's order: (i, ucnt | flags | participates << 31,
                        // key_off[i], key_off[i + 1])
  uint32_t* tsum;       // [n][tiles] tile sums -> exclusive tile offsets
  uint2* kv;            // [n][U] the pair sequences, (key | is_set << 27 | leader << 28, pair index)
};

__global__ void __launch_bounds__(256) k_mk_prep(const EpxState st, const MkBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int u = 0, not_one = 0;
  if (i < b.m) {
    const int P = b.off[b.m], lo = b.off[i], hi = b.off[i + 1];
    if (i == 0) b.info[2] = P;
    bool ok = lo >= 0 && lo <= hi && hi <= P && (i > 0 || lo == 0) && (hi == lo || b.keys);
    // distinct keys: a command is short, so each key is compared with the ones before it (a long list is slow, not wrong)
    for (int j = lo; ok && j < hi; ++j) {
      const int k = b.keys[j];
      ok = k >= 0 && k < st.num_keys;
      bool first = true;
      for (int q = lo; first && q < j; ++q) first = b.keys[q] != k;
      u += first ? 1 : 0;
    }
    if (!ok) {
      epx_report(st.status, FPX_EINVAL, i);
      u = 0;
    }
    b.ucnt[i] = u;
    not_one = hi - lo != 1;
  }
  // per-workgroup partial sums (one address hit by every wavefront's atomics cost ~0.4 ms at 2^20 commands)
  // (both sums behind ONE barrier and no barrier after it; two block_reduce calls were measurably slower in this kernel,
  // which has little else to do: profiles/epaxos_primitives.md, "Speed")
  __shared__ int sh[8];
  u = wave_reduce<ScanSum>(u), not_one = wave_reduce<ScanSum>(not_one);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = u, sh[4 + (threadIdx.x >> 6)] = not_one;
  __syncthreads();
  if (threadIdx.x == 0)
    b.part[blockIdx.x] = make_int2(sh[0] + sh[1] + sh[2] + sh[3], sh[4] + sh[5] + sh[6] + sh[7]);
}

// one workgroup: the partial sums -> info[0..1]; info[3] = the status word, so the host reads one line
__global__ void __launch_bounds__(256) k_mk_total(const EpxState st, const MkBatch b, int blocks) {
  __shared__ int sh[4];
  int u = 0, not_one = 0;
  for (int j = threadIdx.x; j < blocks; j += 256) u += b.part[j].x, not_one += b.part[j].y;
  u = block_reduce<ScanSum, 256>(u, sh), not_one = block_reduce<ScanSum, 256>(not_one, sh);
  if (threadIdx.x == 0) b.info[0] = u, b.info[1] = not_one, b.info[3] = st.status[0];
}

// the pairs keys[lo .. hi) of one command with instance number x
__device__ __forceinline__ void mk_command_pairs(const int32_t* keys, int lo, int hi, int x, uint8_t* uniq, int32_t* pnum) {
  for (int j = lo; j < hi; ++j) {
    const int k = keys[j];
    bool first = true;
    for (int q = lo; first && q < j; ++q) first = keys[q] != k;
    uniq[j] = first ? 1 : 0;
    pnum[j] = x;
  }
}

__global__ void __launch_bounds__(256) k_mk_pairs(const MkBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  mk_command_pairs(b.keys, b.off[i], b.off[i + 1], b.number[i], b.uniq, b.pnum);
}

// k_epx_keys' checks, and the command's record at its position in every replica's order
__global__ void __launch_bounds__(256) k_mk_place(const EpxState st, const MkBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n;
  const int L = b.leader[i];
  const unsigned mask = b.resp_mask[i];
  bool ok = L >= 0 && L < n && b.number[i] >= 0;
  ok = ok && !((mask >> (ok ? L : 0)) & 1u) && (mask >> n) == 0 && (int)__popc(mask) == n - 2;
  const unsigned seen = b.seen_mask ? b.seen_mask[i] : mask;
  ok = ok && (mask & ~seen) == 0 && !((seen >> (ok ? L : 0)) & 1u) && (seen >> n) == 0;
  if (ok && st.num_instances > 0) {  // the `cmdLog.get(instance) == None` branch only, as k_epx_keys
    ok = b.number[i] < st.num_instances;
    const unsigned part = seen | (1u << L);
    for (int r = 0; ok && r < n; ++r)
      if (((part >> r) & 1u) && st.cl_status[((size_t)r * n + L) * st.num_instances + b.number[i]] != CL_NONE) ok = false;
  }
  const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)(ok ? L : 0) << EPX_LEADER_SHIFT) |
                         (uint32_t)b.ucnt[i];
  for (int r = 0; ok && r < n; ++r) {
    const int p = b.rank[(size_t)r * b.m + i];
    ok = p >= 0 && p < b.m;
    const bool part = r == L || ((seen >> r) & 1u);
    if (ok) b.rec[(size_t)r * b.m + p] = make_int4(i, (int)(flags | (part ? 1u << 31 : 0u)), b.off[i], b.off[i + 1]);
  }
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
}

__global__ void __launch_bounds__(256) k_mk_tilesum(const MkBatch b) {
  __shared__ int sh[4];
  const int r = blockIdx.y, t = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 0; k < MK_TILE / 256; ++k) {
    const int p = t * MK_TILE + k * 256 + threadIdx.x;
    if (p < b.m) s += (int)((uint32_t)b.rec[(size_t)r * b.m + p].y & MK_U_MASK);
  }
  s = block_reduce<ScanSum, 256>(s, sh);
  if (threadIdx.x == 0) b.tsum[(size_t)r * b.tiles + t] = (uint32_t)s;
}

// one workgroup per replica: the tile sums -> exclusive tile offsets, in place
__global__ void __launch_bounds__(256) k_mk_tilescan(const MkBatch b) {
  __shared__ uint32_t lds[SCAN_ARRAY_LDS(256)];
  scan_array_excl<ScanSum, 256, 1>(b.tsum + (size_t)blockIdx.x * b.tiles, b.tiles, lds);
}

// thread = 4 consecutive positions of one replica's order: the exclusive offsets inside the tile, then the command's
// distinct keys at offset, offset + 1, ...  Also the rank check of K5 (a position must hold a command of THIS tick whose
// rank is that position: a record left from an earlier tick fails it, see RsArgs::rank), so the writes below are bounded
// by U whatever the ranks were.
__global__ void __launch_bounds__(256) k_mk_scatter(const EpxState st, const MkBatch b) {
  __shared__ uint32_t sh[4];
  const int r = blockIdx.y, t = blockIdx.x, p0 = t * MK_TILE + threadIdx.x * 4;
  int4 rc[4];
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = p0 + k;
    rc[k] = p < b.m ? b.rec[(size_t)r * b.m + p] : make_int4(-1, 0, 0, 0);
    s += (uint32_t)rc[k].y & MK_U_MASK;
  }
  uint32_t base = block_excl_scan<ScanSum, 256>(s, b.tsum[(size_t)r * b.tiles + t], sh);
  uint2* out = b.kv + (size_t)r * b.U;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = p0 + k;
    if (p >= b.m) break;
    const int i = rc[k].x;
    const uint32_t w = (uint32_t)rc[k].y, u = w & MK_U_MASK;
    if (i < 0 || i >= b.m || b.rank[(size_t)r * b.m + i] != p || (uint64_t)base + u > (uint64_t)b.U) {
      bad = true;
      break;
    }
    const uint32_t flags = w & (0xFu << EPX_SET_SHIFT);
    const bool part = w >> 31;
    uint32_t q = base;
    for (int j = imax(rc[k].z, 0); j < rc[k].w && j < b.P && q < base + u; ++j)
      if (b.uniq[j]) out[q++] = make_uint2((part ? (uint32_t)b.keys[j] : (uint32_t)st.num_keys) | flags, (uint32_t)j);
    base += u;
  }
  if (bad) epx_report(st.status, FPX_EINVAL, -1);
}

// conf row of (command i, replica r) = the max over the rows of the command's distinct-key pairs, for the replicas that
// scanned the command (the tick: its leader and seen_mask; K7: the replicas that processed it)
struct MkMerge {
  int m;
  const int32_t* off;
  const uint8_t* uniq;
  const int32_t* pconf;  // [P][n][NP]
  int32_t* conf;         // [m][n][NP]
  const int32_t* leader;
  const uint8_t* resp_mask;
  const uint8_t* seen_mask;
  const uint8_t* act;    // K7: [n][m] (replica r scanned message i iff act == HP_PROCESS); null: the tick
};

template <int N>
__global__ void __launch_bounds__(256) k_mk_merge(const EpxState st, const MkMerge b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  constexpr int NP = ConfRow<N>::NP;
  unsigned part = 0;
  if (b.act) {
    for (int r = 0; r < N; ++r) part |= (b.act[(size_t)r * b.m + i] == HP_PROCESS ? 1u : 0u) << r;
  } else {
    part = (b.seen_mask ? b.seen_mask[i] : b.resp_mask[i]) | (1u << b.leader[i]);
  }
  const int lo = b.off[i], hi = b.off[i + 1];
  for (int r = 0; r < N; ++r) {
    if (!((part >> r) & 1u)) continue;
    int4 a0 = make_int4(0, 0, 0, 0), a1 = make_int4(0, 0, 0, 0);
    for (int j = lo; j < hi; ++j) {
      if (!b.uniq[j]) continue;
      const int4* row = reinterpret_cast<const int4*>(b.pconf + ((size_t)j * N + r) * NP);
      const int4 x = row[0];
      a0 = make_int4(imax(a0.x, x.x), imax(a0.y, x.y), imax(a0.z, x.z), imax(a0.w, x.w));
      if constexpr (NP == 8) {
        const int4 y = row[1];
        a1 = make_int4(imax(a1.x, y.x), imax(a1.y, y.y), imax(a1.z, y.z), imax(a1.w, y.w));
      }
    }
    int4* dst = reinterpret_cast<int4*>(b.conf + ((size_t)i * N + r) * NP);
    dst[0] = a0;
    if constexpr (NP == 8) dst[1] = a1;
  }
}
