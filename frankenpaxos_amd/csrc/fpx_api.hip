// fpx_api.hip -- the C ABI of include/fpx.h on top of the gfx950 kernels in fpx_kernels.hpp.
//
// There is NO CPU path in this file: every entry point that computes anything launches a HIP kernel
// and fails with FPX_ENODEVICE / FPX_EHIP when no device is usable.
#include "../../include/fpx.h"

#include <dlfcn.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "fpx_host.hpp"
#include "fpx_kernels.hpp"
#include "fpx_phase1_info.hpp"
#include "fpx_phase1b_msgs.hpp"
#include "fpx_ranges.hpp"
#include "fpx_tally_msgs.hpp"
#include "fpx_mencius_msgs.hpp"
#include "fpx_replica_msgs.hpp"
#include "fpx_burst_sort.hpp"
#include "fpx_replica_inbox.hpp"
#include "fpx_acceptor_inbox.hpp"
#include "fpx_mencius_acceptor_inbox.hpp"
#include "fpx_wire_dev.hpp"
#include "fpx_wire_enc_dev.hpp"
#include "../../include/fpx_wire.h"

using namespace fpx;

// RCCL is bound at run time (dlopen), never at link time: a process that already carries an RCCL (PyTorch
// bundles its own librccl.so) must keep using THAT copy -- two RCCLs in one address space do not share their
// communicator state -- and a single-GPU caller needs no RCCL at all.  The handful of types below mirror
// rccl.h (NCCL 2.x ABI: ncclUniqueId is 128 opaque bytes, ncclSum = 0, ncclUint64 = 5, ncclSuccess = 0).
struct RcclUniqueId { char internal[128]; };
typedef void* RcclComm;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(RcclUniqueId*) = nullptr;
  int (*CommInitRank)(RcclComm*, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(RcclComm) = nullptr;
  int (*ReduceScatter)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, RcclComm, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;  // optional: several collectives as one launch (fpx_comm_allgather_chosen_dev)
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static_assert(sizeof(RcclUniqueId) == FPX_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
enum { RCCL_SUM = 0, RCCL_MAX = 2, RCCL_UINT8 = 1, RCCL_INT32 = 2, RCCL_UINT64 = 5 };  // ncclRedOp_t / ncclDataType_t values

// One call in flight: staging buffers for its inputs, two events, a page-locked copy of the status words taken right after
// its fused step.
constexpr int HOST_DEPTH = 3;
struct HostSlot {
  DevBuf in[4];               // the call's inputs staged in HBM (validation and the vote kernel read them there)
  DevBuf sink[3];             // where the records go that the caller did not ask for (a null output array)
  hipEvent_t up = nullptr;    // the inputs are up (the copy engine's stream)
  hipEvent_t done = nullptr;  // validation + fused step + status snapshot are done: the records are in the caller's arrays
  int32_t* status = nullptr;  // page-locked, 8 words: the device's status right after the call (k_status_snap)
  int32_t* status_dev = nullptr;
  bool busy = false;          // submitted, not waited for yet
  int n = 0;
};

struct fpx_ctx {
  fpx_config cfg;
  Geom g;
  State st;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  int lanes_per_slot = 64;  // G
  bool vec = false;
  int num_cus = 256;
  int max_grid = 2048;
  uint32_t run_id = 0;
  int64_t bytes = 0;
  int last_hip = 0;
  int32_t err_index = -1, err_slot = -1, err_round = -1;
  // Host-pointer entry points: every array of a call -- inputs, outputs, device-only temporaries -- is carved out of ONE
  // staging buffer by the driver the EPaxos context shares (host_call, fpx_host.hpp); an entry point lists its arrays and
  // the list points its typed slots at them.  No array of a host form has a buffer of its own in this struct.
  HostStage stage;
  DevBuf d_scratch;  // the few words (or the one dump) that a read-back entry point, Phase 1 included, copies out itself
  // host-side run splitting
  std::vector<uint32_t> hstamp;
  uint32_t hrun = 0;
  std::vector<int32_t> hround;
  // kernel timing (fpx_profile_*)
  void* slab = nullptr;  // vote_round | vote_value | ballot
  // chunk placement (place_chunks): the slab is a reserved address range backed by 1 GiB physical allocations
  std::vector<hipMemGenericAllocationHandle_t> vmm_chunks;  // the chunks mapped into the slab, in address order
  size_t vmm_reserved = 0;                                  // bytes of the reservation at `slab` (0: the slab is one hipMalloc)
  int placement_probes = 0, placement_unprobed = 0;          // the search itself: probes run, decisions taken unprobed (budget spent)
  float placement_ms = 0.f;                                 // wall clock of the search
  float placement[5] = {0, 0, 0, 0, 0};                     // mode (0 one allocation, 1 chunks), windows, min / median / max probe ms
  uint32_t phase2_launches = 0;
  int lz_min_from = 0x7fffffff;     // the smallest watermark of any Phase1a since the lazy records were last cleared: a Phase1a whose
                                    // watermark is not above it cannot meet an older record that starts below its own (k_p1a_fast)
  // the fold (k_finalize's work) of the last K3 launch, when it has not been launched: it rides in the next eligible vote
  // kernel (k_phase2_fin) or is launched by whatever touches the context next (DeviceGuard -> flush_pending_fin)
  FinJob pending_fin = {};       // nblk != 0: pending
  long long fins_carried = 0;    // diagnostic
  uint32_t launch_seq = 0;  // stamps the partial-maxima rows of a K1 / K3 launch (never 0 in a row that counts)
  bool profiling = false;
  std::vector<hipEvent_t> ev;  // start/stop pairs
  size_t ev_used = 0;
  // host-pointer K3 on page-locked arrays: the inputs go up on a stream of their own (host_submit)
  hipStream_t up_stream = nullptr;
  HostSlot* hslots = nullptr;  // calls in flight on page-locked arrays (host_submit / host_wait)
  int hnext = 0;
  bool lazy_active = false;  // PER_SLOT: lazy Phase1a promises may be outstanding (k_phase2 runs its lazy-aware form)
  bool may_compact = false;  // some vote row may be ROW_COMPACT: a steady walk may have run since all rows were last fresh or cells
  DevBuf d_run_done;         // one byte per chunk: taken by the packed walk
  // K4: the proxy leader's noop-range tallies (two buffers: fpx_proxy_forget rehashes into the other one)
  RangeTable rt[2];
  int rt_cur = 0;
  DevBuf d_rng;     // scratch of device range batches (fpx_noop_ranges_fused_dev)
  // fpx_mencius_band_fused_dev: the ranges' half of an independent step runs here, between a fork and a join event
  hipStream_t band_stream = nullptr;
  int64_t band_merged_steps = 0;
  hipEvent_t band_fork = nullptr, band_join = nullptr;
  // fpx_vote_launch_census (include/fpx.h): host counters of the vote launches and of their folds
  int64_t census[FPX_CENSUS_WORDS] = {};
  int census_pending = 0;  // the cell of the launch whose fold is pending_fin
  int64_t range_census[FPX_RANGE_CENSUS_WORDS] = {};  // fpx_range_launch_census: host counters of the K4 launches
  DevBuf d_enc;   // the device encoders' workgroup sums (fpx_wire_encode_*_dev)
  // fpx_proxy_phase2b_msgs_dev (fpx_tally_msgs.hpp): the owner word of every tally entry ([S][wp], INT_MAX between calls;
  // allocated by the first call), and per call the messages' entries and the gathered rows
  DevBuf m_owner, m_entry, m_rows;
  // fpx_mencius_proxy_phase2b_msgs_dev (fpx_mencius_msgs.hpp): the claim word of every range-table entry ([cap], INT_MAX
  // between calls; allocated by the first call; one array for both table buffers)
  DevBuf mm_claim;
  // fpx_replica_chosen_msgs_dev (fpx_replica_msgs.hpp): the claim word of every slot ([S], INT_MAX between calls; allocated
  // by the first call), and per call the header words, the workgroups' folds, and the list of the burst's ranges
  DevBuf rm_claim, rm_buf;
  // fpx_replica_inbox[_dev] (fpx_replica_inbox.hpp): the per-call scratch (header words, the workgroups' folds, the tiles'
  // maxima, the sort's counts and its two key / value buffers).  The claim words are rm_claim's.
  DevBuf ri_buf;
  // fpx_acceptor_inbox[_dev] (fpx_acceptor_inbox.hpp): the per-call scratch (header words, the tiles' maxima, the sort's
  // counts and its two key / value buffers, the accepted slots and claim positions, the entries' new scalars), and the claim
  // table sized by the largest burst so far (cell numbers, all ones between calls; bids, -1 between calls)
  DevBuf ai_buf, ai_tkey, ai_tval;
  // fpx_mencius_acceptor_inbox[_dev] (fpx_mencius_acceptor_inbox.hpp): the per-call scratch (ai_buf's parts, the range
  // flags, the tiles' range counts and the list of accepted ranges).  The claim table is ai_*'s.
  DevBuf mai_buf;
  // fpx_acceptor_phase1b_info_all[_dev] (fpx_phase1_info.hpp): the chunk counts, column totals and the go word
  DevBuf p1i;
  // fpx_leader_phase1b_msgs[_dev] (fpx_phase1b_msgs.hpp): the per-call scratch (control block, first / last tables, the
  // winners' work list), and the bid table (cap x 8 bytes)
  DevBuf p1m_buf, p1m_tab;
  DevBuf d_band;  // [num_leader_groups] marks: the leader groups with a range in the step being checked
  // multi-GPU (fpx_comm_*): one communicator per context, rank = this context's GPU
  RcclComm comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  int last_rccl = 0;
  DevBuf d_part, d_mine;       // partial vote bitmaps of my acceptors (all slots) / full bitmaps of my slots
  std::vector<hipEvent_t> cev;  // start/stop pairs around the collective
  size_t cev_used = 0;
};

namespace {

// Every entry point runs inside a DeviceScope (fpx_host.hpp) of the context's device.
void flush_pending_fin(fpx_ctx* ctx);
struct DeviceGuard : DeviceScope {
  explicit DeviceGuard(int device) : DeviceScope(device) {}
  // Every entry point that takes the context starts here; all but fpx_phase2_fused_dev (which enters by device number
  // and deals with a pending fold itself) first launch the fold of the last K3 launch if it is still pending -- so
  // nothing that reads or moves the acceptors' scalars ever sees them short of a launch (see k_phase2_fin).
  explicit DeviceGuard(const fpx_ctx* ctx) {
    if (!ctx) return;
    enter(ctx->cfg.device);
    if (ctx->pending_fin.nblk) flush_pending_fin(const_cast<fpx_ctx*>(ctx));
  }
};

int check_config(const fpx_config* c) {
  if (!c) return FPX_EINVAL;
  if (c->num_slots < 1) return FPX_EINVAL;
  if (c->num_replicas < 1 || c->num_replicas > FPX_MAX_REPLICAS) return FPX_EINVAL;
  if (c->num_groups < 1 || c->num_leader_groups < 1) return FPX_EINVAL;
  if (c->num_leaders < 1) return FPX_EINVAL;
  if (c->tally_ways < 1 || c->tally_ways > 8) return FPX_EINVAL;
  if (c->ballot_mode != FPX_BALLOT_ACCEPTOR && c->ballot_mode != FPX_BALLOT_PER_SLOT) return FPX_EINVAL;
  const int total = c->replicas_total ? c->replicas_total : c->num_replicas;
  if (total < 1 || total > FPX_MAX_REPLICAS) return FPX_EINVAL;
  if (c->replica_base < 0 || (c->replica_base & 3) || c->replica_base + c->num_replicas > total) return FPX_EINVAL;
  // the per-block maxima tables live in LDS
  if ((int64_t)c->num_groups * c->num_leader_groups * c->num_replicas > 8192) return FPX_EINVAL;
  switch (c->quorum_kind) {
    case FPX_Q_THRESHOLD:
      if (c->f < 0 || c->f + 1 > total) return FPX_EINVAL;
      break;
    case FPX_Q_SIMPLE_MAJORITY:
    case FPX_Q_UNANIMOUS:
      break;
    case FPX_Q_GRID:
      if (c->grid_rows < 1 || c->grid_cols < 1 || c->grid_rows * c->grid_cols != total) return FPX_EINVAL;
      break;
    default:
      return FPX_EINVAL;
  }
  return FPX_OK;
}

// the row of slot s in the cell arrays and tally tables (device: phys_slot)
static inline size_t host_phys_slot(const Geom& g, int s) {
  return g.lg_rows ? (size_t)(s % g.num_leader_groups) * g.lg_rows + (size_t)(s / g.num_leader_groups) : (size_t)s;
}

void make_geom(const fpx_config& c, Geom* g) {
  memset(g, 0, sizeof(*g));
  g->S = c.num_slots;
  g->R = c.num_replicas;
  g->RS = (c.num_replicas + 3) & ~3;
  // small groups (R <= 4): the vote round and vote value rows of a slot share one 32-byte sector
  { const char* il = getenv("FPX_INTERLEAVE"); g->VS = (g->RS == 4 && il && atoi(il) != 0) ? 8 : g->RS; }
  g->num_groups = c.num_groups;
  g->num_leader_groups = c.num_leader_groups;
  g->ngroups = c.num_groups * c.num_leader_groups;
  // Mencius: rows leader-group-major when the window is a whole number of rounds over the leader groups
  g->lg_rows = (c.num_leader_groups > 1 && c.num_slots % c.num_leader_groups == 0 && c.num_replicas <= 32 &&
                !(c.flags & FPX_F_SLOT_MAJOR_ROWS) && !getenv("FPX_SLOT_MAJOR"))
                   ? c.num_slots / c.num_leader_groups : 0;
  // slot / L and row / A by multiplication (fpx_fastdiv.hpp)
  fast_div_magic(c.num_leader_groups, &g->l_magic, &g->l_shift);
  fast_div_magic(c.num_groups, &g->a_magic, &g->a_shift);
  g->qkind = c.quorum_kind;
  g->total = c.replicas_total ? c.replicas_total : c.num_replicas;
  g->base = c.replica_base;
  switch (c.quorum_kind) {
    case FPX_Q_THRESHOLD: g->qsize = c.f + 1; break;                 // ProxyLeader.scala:238
    case FPX_Q_SIMPLE_MAJORITY: g->qsize = g->total / 2 + 1; break;  // SimpleMajority.scala:30
    case FPX_Q_UNANIMOUS: g->qsize = g->total; break;                // UnanimousWrites.scala:50
    default: g->qsize = 0;
  }
  g->grid_rows = c.grid_rows;
  g->grid_cols = c.grid_cols;
  g->per_slot = c.ballot_mode == FPX_BALLOT_PER_SLOT;
  g->ways = c.tally_ways;
  g->wp = c.tally_ways <= 4 ? 4 : 8;
  for (int w = 0; w < 4; ++w) {
    const int lo = w * 64;
    g->member[w] = g->total >= lo + 64 ? ~0ull : (g->total <= lo ? 0ull : ((1ull << (g->total - lo)) - 1ull));
  }
}

// grow() for a buffer that fpx_device_bytes counts
int grow_counted(fpx_ctx* ctx, DevBuf* b, size_t bytes) {
  const size_t had = b->cap;
  const int rc = grow(ctx, b, bytes);
  ctx->bytes += (int64_t)b->cap - (int64_t)had;
  return rc;
}

// carve() for a buffer that fpx_device_bytes counts
template <typename S, typename Lay>
int carve_counted(fpx_ctx* ctx, DevBuf* buf, S* out, Lay lay) {
  const size_t had = buf->cap;
  const int rc = carve(ctx, buf, out, lay);
  ctx->bytes += (int64_t)buf->cap - (int64_t)had;
  return rc;
}

template <typename T>
int dalloc(fpx_ctx* ctx, T** p, size_t count) {
  HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
  ctx->bytes += (int64_t)(count * sizeof(T));
  return FPX_OK;
}

size_t lds_bytes(const fpx_ctx* ctx, bool fused, bool targets) {
  const size_t tab = (((size_t)ctx->g.ngroups * ctx->g.R * 8) + 16 + 15) & ~(size_t)15;  // tables + 4 workgroup words
  // (targets: per wavefront the chunk's 64 masks + 16 words for the packed walk's Nack path)
  return tab + 4 * (fused ? sizeof(WaveOut<true>) : sizeof(WaveOut<false>)) + (targets ? 4 * (256 + 16) * sizeof(uint64_t) : 0);
}

// messages per wavefront at G = 64: CHUNK (CHUNK_RECORDS) for batches that fill the chip anyway, fewer (down to 4) for small
// ones -- a wave walks its chunk one row at a time, so a 20 k-message epoch in 32-message chunks is 670 waves
// walking 32 dependent steps each on a machine with room for 6000
int chunk_for(const fpx_ctx* ctx, int n) {
  if (ctx->lanes_per_slot != 64) return 64;
  // (the floor: the sweep of profiles/r06_raw/adversarial_chunk_sweep.txt -- 8 / 4 / 2 / 1 messages per wavefront at ~21 500
  // messages per launch: 6.12 / 6.50 / 6.55 / 6.53e8 proposals/s; 4 stays)
  const long long want_waves = (long long)ctx->num_cus * 16;
  // (records are kept AND written: the steady walk needs one acceptor group; with several every row still stores its cells)
  int ch = ctx->st.vote_sum && ctx->g.ngroups == 1 ? CHUNK_RECORDS : CHUNK;
  while (ch > 4 && (long long)(n + ch - 1) / ch < want_waves) ch >>= 1;
  return ch;
}

int grid_for(const fpx_ctx* ctx, int n) {
  const int per_block = 4 * chunk_for(ctx, n);
  const int need = (n + per_block - 1) / per_block;
  return std::max(1, std::min(need, ctx->max_grid));
}

// dynamic LDS above the 64 KiB default needs an opt-in per kernel (gfx950 has 160 KiB per CU): the maxima
// tables of a context with thousands of acceptors (num_groups * num_leader_groups * R up to 8192) reach 83 KiB
template <typename K>
void allow_lds(K kernel, size_t lds) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// dynamic LDS of one vote-kernel launch; the offsets of its optional parts go into the batch
size_t phase2_lds(fpx_ctx* ctx, Batch& b, bool fused, bool targets, bool acceptor_rounds) {
  size_t lds = lds_bytes(ctx, fused, targets);
  // leader-group-major rows: 3 KiB of LDS per wavefront for the column quads of a slot-ordered batch (k_phase2), when
  // every array they move as 16 bytes is aligned for it
  auto al = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  if (ctx->g.lg_rows && al(b.slot, 16) && al(b.round, 16) && al(b.value, 16) && al(b.chosen, 4) && al(b.chosen_round, 16) &&
      al(b.chosen_value, 16) && al(b.nack_round, 16)) {
    lds = (lds + 15) & ~(size_t)15;
    b.sc_lds = (int32_t)lds;
    lds += 4 * 3 * 4 * 64 * sizeof(int32_t);
  }
  if (acceptor_rounds && ctx->g.ngroups != 1) {  // the acceptors' rounds of every group, staged per workgroup
    lds = (lds + 15) & ~(size_t)15;
    b.th_lds = (int32_t)lds;
    lds += (size_t)ctx->g.ngroups * ctx->g.R * sizeof(int32_t);
  }
  return lds;
}

// one vote launch in its census cell (fpx_vote_launch_census); returns the cell
int census_launch(fpx_ctx* ctx, int G, int mode, int ps, bool fused, int form, const Batch& b) {
  const int cell = FPX_CENSUS_CELL(__builtin_ctz((unsigned)G), mode, ps, fused ? 1 : 0);
  ++ctx->census[cell * FPX_CENSUS_FORMS + form];
  if (b.sc_lds) ++ctx->census[FPX_CENSUS_SC_LDS];
  if (b.th_lds) ++ctx->census[FPX_CENSUS_TH_LDS];
  return cell;
}
void census_fold(fpx_ctx* ctx, int cell, int fate) { ++ctx->census[cell * FPX_CENSUS_FORMS + fate]; }

// One K1 / K3 kernel launch, as enqueue_phase2 / enqueue_band_merged hand it down the launch chain.
struct VoteLaunch {
  State st;             // the State the launch runs on: ctx->st with ITS half of part / part_stamp (begin_phase2_launch)
  FinJob fin = {};      // the fold of the launch before, offered to this one (nblk != 0): taken into its grid when the
  int fin_cell = 0;     // kernel has that form (k_phase2_fin); fin_cell: the census cell of the launch it folds
  // the events ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL), so a timed launch puts no marker packets
  // on the stream (two hipEventRecords per launch cost 5 - 15 us of a step)
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  bool packed = false;  // the packed walk over runs of acceptors (k_phase2 MODE 3)
};
struct Launched { int cell; bool took_fin; };  // what a launch did: its census cell, whether it took VoteLaunch::fin along

template <int G, int MODE, int PS>
Launched launch_phase2_3(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b0, bool fused, int grid) {
  Batch b = b0;
  const size_t lds = phase2_lds(ctx, b, fused, MODE != 0, PS == 0);
  if (fused) allow_lds(k_phase2<G, MODE, PS, true>, lds);
  else allow_lds(k_phase2<G, MODE, PS, false>, lds);
  if constexpr ((G == 64 || G == 1) && (MODE == 0 || MODE == 2) && PS != 0) {
    // the fold of the launch before rides in this one (k_phase2_fin: the shapes of the steady streams -- the headline,
    // configs 2 and 3, the adversarial stream; other shapes leave it to the caller, who launches it by itself)
    if (fused && vl.fin.nblk) {
      allow_lds(k_phase2_fin<G, MODE, PS, true>, lds);
      hipExtLaunchKernelGGL((k_phase2_fin<G, MODE, PS, true>), dim3(grid + vl.fin.nblk), dim3(256), (uint32_t)lds, ctx->stream,
                            vl.ev_start, vl.ev_stop, 0, ctx->g, vl.st, b, vl.fin);
      ++ctx->fins_carried;
      census_fold(ctx, vl.fin_cell, FPX_CENSUS_FOLD_CARRIED);
      return {census_launch(ctx, G, MODE, PS, fused, FPX_CENSUS_FIN, b), true};
    }
  }
  if (fused)
    hipExtLaunchKernelGGL((k_phase2<G, MODE, PS, true>), dim3(grid), dim3(256), (uint32_t)lds, ctx->stream, vl.ev_start,
                          vl.ev_stop, 0, ctx->g, vl.st, b);
  else
    hipExtLaunchKernelGGL((k_phase2<G, MODE, PS, false>), dim3(grid), dim3(256), (uint32_t)lds, ctx->stream, vl.ev_start,
                          vl.ev_stop, 0, ctx->g, vl.st, b);
  return {census_launch(ctx, G, MODE, PS, fused, b.solo ? FPX_CENSUS_SOLO : FPX_CENSUS_GRID, b), false};
}

template <int G, int MODE>
Launched launch_phase2_2b(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b, bool fused, int grid) {
  // ballot model: 0 = per-acceptor scalar, 1 = per cell, 2 = per cell with lazy Phase1a promises outstanding
  if (!ctx->g.per_slot) return launch_phase2_3<G, MODE, 0>(ctx, vl, b, fused, grid);
  if (!ctx->lazy_active) return launch_phase2_3<G, MODE, 1>(ctx, vl, b, fused, grid);
  return launch_phase2_3<G, MODE, 2>(ctx, vl, b, fused, grid);
}

template <int G>
Launched launch_phase2_2(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b, bool fused, int grid) {
  // rows are padded to a multiple of 4 cells (Geom::RS), so int4 accesses serve every R.
  // mode 0: dense delivery (no target masks); 1: target masks; 2: target masks + FPX_F_SCATTERED_TARGETS
  const int mode = !b.target ? 0 : ((ctx->cfg.flags & FPX_F_SCATTERED_TARGETS) ? 2 : 1);
  if constexpr (G == 64) {
    if (vl.packed) {  // the packed walk (enqueue_phase2 runs it ahead of the row-at-a-time walk)
      if (!ctx->g.per_slot) return launch_phase2_3<64, 3, 0>(ctx, vl, b, fused, grid);
      return launch_phase2_3<64, 3, 1>(ctx, vl, b, fused, grid);
    }
  }
  if (mode == 0) return launch_phase2_2b<G, 0>(ctx, vl, b, fused, grid);
  if (mode == 1) return launch_phase2_2b<G, 1>(ctx, vl, b, fused, grid);
  return launch_phase2_2b<G, 2>(ctx, vl, b, fused, grid);
}

Launched launch_phase2(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b, bool fused, int grid) {
  switch (ctx->lanes_per_slot) {
    case 1: return launch_phase2_2<1>(ctx, vl, b, fused, grid);
    case 2: return launch_phase2_2<2>(ctx, vl, b, fused, grid);
    case 4: return launch_phase2_2<4>(ctx, vl, b, fused, grid);
    case 8: return launch_phase2_2<8>(ctx, vl, b, fused, grid);
    case 16: return launch_phase2_2<16>(ctx, vl, b, fused, grid);
    case 32: return launch_phase2_2<32>(ctx, vl, b, fused, grid);
    default: return launch_phase2_2<64>(ctx, vl, b, fused, grid);
  }
}

// the vote kernel of a Mencius band with the band's range chain as its first workgroup (enqueue_band_merged)
template <int G>
void launch_band_g(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b, size_t lds, int grid, const RangeBatch& rb) {
  allow_lds(k_phase2_band<G, 0, 0, true>, lds);
  census_launch(ctx, G, 0, 0, true, FPX_CENSUS_BAND, b);
  hipExtLaunchKernelGGL((k_phase2_band<G, 0, 0, true>), dim3(grid + 1), dim3(256), (uint32_t)lds, ctx->stream, vl.ev_start,
                        vl.ev_stop, 0, ctx->g, vl.st, b, ctx->rt[ctx->rt_cur], rb);
}
void launch_band(fpx_ctx* ctx, const VoteLaunch& vl, const Batch& b, size_t lds, int grid, const RangeBatch& rb) {
  switch (ctx->lanes_per_slot) {
    case 1: launch_band_g<1>(ctx, vl, b, lds, grid, rb); break;
    case 2: launch_band_g<2>(ctx, vl, b, lds, grid, rb); break;
    case 4: launch_band_g<4>(ctx, vl, b, lds, grid, rb); break;
    default: launch_band_g<8>(ctx, vl, b, lds, grid, rb); break;
  }
}

// fill n int32 words on a stream (the context's, when none is named) with a kernel (see k_fill32)
void fill32(fpx_ctx* ctx, void* p, int32_t v, size_t n, hipStream_t stream) {
  if (n == 0) return;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)ctx->num_cus * 8));
  hipLaunchKernelGGL(k_fill32, dim3(grid), dim3(256), 0, stream, (int32_t*)p, v, n);
}
void fill32(fpx_ctx* ctx, void* p, int32_t v, size_t n) { fill32(ctx, p, v, n, ctx->stream); }

// a claim array of `words` int32 that lives as long as the context: the first call allocates it, counts it and sets
// every word to INT_MAX, its value between calls
int claim_array(fpx_ctx* ctx, DevBuf* b, size_t words) {
  if (b->p) return FPX_OK;
  const int rc = grow_counted(ctx, b, words * 4);
  if (rc) return rc;
  fill32(ctx, b->p, INT_MAX, b->cap / 4);
  return FPX_OK;
}

// What the caller of one device run says about it.  A _dev entry point runs AS_CONFIGURED: validated on the device unless
// the context is FPX_F_TRUSTED.  A host batch run whole is validated even then (FORCE_VALIDATE: that flag is a promise
// about _dev batches only); one that the host cut into runs itself (split_runs) holds the run contract by construction
// and skips the device pass (CUT_ON_HOST).  index_base is the message index of the run in its host batch: error reports
// are batch-relative.
struct RunOpts {
  enum Validate { AS_CONFIGURED, FORCE_VALIDATE, CUT_ON_HOST } validate = AS_CONFIGURED;
  int32_t index_base = 0;
  bool validates(const fpx_ctx* ctx) const {
    return validate == FORCE_VALIDATE || (validate == AS_CONFIGURED && !(ctx->cfg.flags & FPX_F_TRUSTED));
  }
};

// the run's stamp and index base into the batch, then the validation pass of one device run (RunOpts says whether it runs)
int enqueue_validate(fpx_ctx* ctx, Batch& b, bool check_round, const RunOpts& opts) {
  b.run_id = ++ctx->run_id, b.index_base = opts.index_base;
  if (ctx->run_id == 0xFFFFFFFFu) {  // stamp space exhausted: start over
    HIPCHK(ctx, hipMemsetAsync(ctx->st.stamp, 0, sizeof(uint32_t) * (size_t)ctx->g.S, ctx->stream));
    ctx->run_id = 0;
    b.run_id = ++ctx->run_id;
  }
  if (!opts.validates(ctx)) return FPX_OK;
  b.check_round = check_round && !ctx->g.per_slot;
  if (b.check_round) fill32(ctx, ctx->st.run_round, -1, (size_t)ctx->g.ngroups);
  hipLaunchKernelGGL(k_validate, dim3((b.n + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, b);
  return launch_check(ctx);
}

// The launch counter of a K1 / K3 launch decides which third of part_all (Batch::parity) and which half of part /
// part_stamp (the State handed to the launch and to its fold) it uses: see finalize_body / k_phase2_fin.
State begin_phase2_launch(fpx_ctx* ctx, Batch& b) {
  const uint32_t li = ctx->phase2_launches++;
  b.parity = (int32_t)(li % 3u);
  const size_t half = (size_t)(li & 1u), ntab = (size_t)ctx->g.ngroups * ctx->g.R;
  State st = ctx->st;
  st.part = ctx->st.part + half * (size_t)ctx->max_grid * 2 * ntab;
  st.part_stamp = ctx->st.part_stamp + half * (size_t)ctx->max_grid;
  return st;
}

// the fold of the launch of b on `st` (begin_phase2_launch's) over `grid` workgroups
FinJob fin_job_of(const fpx_ctx* ctx, const State& st, const Batch& b, int grid) {
  FinJob fj;
  const int ntab = ctx->g.ngroups * ctx->g.R;
  fj.fgx = (ntab + 63) / 64;
  fj.slices = std::max(FINALIZE_SLICES, std::min(256, grid / 32));  // ~8 partial rows per wavefront
  fj.nblk = fj.fgx * fj.slices;
  fj.par = (int)b.parity, fj.grid = grid, fj.seq = b.launch_seq;
  fj.part = st.part, fj.part_stamp = st.part_stamp;
  return fj;
}

void launch_fin_alone(fpx_ctx* ctx, const FinJob& fj) {
  State fs = ctx->st;
  fs.part = fj.part, fs.part_stamp = fj.part_stamp;
  hipLaunchKernelGGL(k_finalize, dim3(fj.fgx, fj.slices), dim3(256), 0, ctx->stream, ctx->g, fs, fj.par, fj.grid, fj.seq);
}

void flush_pending_fin(fpx_ctx* ctx) {
  if (!ctx->pending_fin.nblk) return;
  launch_fin_alone(ctx, ctx->pending_fin);
  ctx->pending_fin.nblk = 0;
  census_fold(ctx, ctx->census_pending, FPX_CENSUS_FOLD_FLUSHED);
  (void)launch_check(ctx);
}

// K1 / K3 on one device run
int enqueue_phase2(fpx_ctx* ctx, Batch& b, bool fused, const RunOpts& opts) {
  if (b.n == 0) return FPX_OK;
  int rc = enqueue_validate(ctx, b, true, opts);
  if (rc) return rc;
  int grid = grid_for(ctx, b.n);
  b.chunk = chunk_for(ctx, b.n);
  // at most two chunks per wavefront of one workgroup: that workgroup finalises itself (k_phase2, `solo`); the parity
  // of the partial-maxima buffers is not consumed
  b.solo = (b.n + b.chunk - 1) / b.chunk <= 8 ? 1 : 0;
  if (b.solo) grid = 1;
  else if ((b.n + 4 * b.chunk - 1) / (4 * b.chunk) > grid) ++ctx->census[FPX_CENSUS_CAPPED];
  // Target masks on 256-cell rows of one group: thrifty delivery to RUNS of neighbouring acceptors (what GpuProxyLeader
  // sends by default; any f + 1 will do: ProxyLeader.scala:190-191) takes two rows per wavefront step.  Two launches: the
  // packed walk takes the chunks all of whose messages go to such runs of rows nobody voted in yet and marks them, the
  // row-at-a-time walk behind it takes the rest (nothing is decided on the host, nothing is walked twice).
  const Geom& g = ctx->g;
  const bool two = b.target && ctx->lanes_per_slot == 64 && g.RS == 256 && g.ngroups == 1 && g.base == 0 && g.total == g.R &&
                   g.qkind != 2 && !(g.per_slot && ctx->lazy_active) && !(ctx->cfg.flags & FPX_F_SCATTERED_TARGETS) &&
                   !getenv("FPX_NO_PACKED_RUNS");  // (FPX_F_SCATTERED_TARGETS: the caller says its targets are no runs)
  if (two) {
    rc = grow(ctx, &ctx->d_run_done, (size_t)(b.n + b.chunk - 1) / b.chunk + 64);
    if (rc) return rc;
    b.run_done = (uint8_t*)ctx->d_run_done.p;
  }
  // Vote-row records.  Only a dense launch (its steady walk) writes them, and only the dense kernels read them: in front of a launch that carries target masks the compact rows among its slots become
  // cells (k_expand_batch; an undelivered message's row too, which changes no cell's value) -- while there may be any.
  // A stream of such launches alone (the adversarial one) never pays the launch
  if (ctx->st.vote_sum) {
    if (!b.target) {
      if (g.ngroups == 1) ctx->may_compact = true;
    } else if (ctx->may_compact) {
      const int ge = (int)std::min<long long>(((long long)b.n + 3) / 4, (long long)ctx->num_cus * 8);
      hipLaunchKernelGGL(k_expand_batch, dim3(ge), dim3(256), 0, ctx->stream, ctx->g, ctx->st, b.slot, b.n);
      if ((rc = launch_check(ctx))) return rc;
    }
  }
  const bool prof = ctx->profiling && ctx->ev_used + 2 <= ctx->ev.size();
  for (int pass = two ? 0 : 1; pass < 2; ++pass) {
    // start of the first vote kernel to end of the last (two with the packed walk ahead)
    VoteLaunch vl;
    vl.ev_start = prof && pass == (two ? 0 : 1) ? ctx->ev[ctx->ev_used] : nullptr;
    vl.ev_stop = prof && pass == 1 ? ctx->ev[ctx->ev_used + 1] : nullptr;
    if (b.solo) {
      // (the one workgroup of a solo launch raises the acceptors' scalars with plain loads and stores: nothing may fold
      // beside it -- a pending fold goes first, by itself)
      flush_pending_fin(ctx);
      b.parity = 0, vl.st = ctx->st;
    } else {
      vl.st = begin_phase2_launch(ctx, b);
    }
    if (++ctx->launch_seq == 0) ctx->launch_seq = 1;
    b.launch_seq = ctx->launch_seq;
    vl.packed = pass == 0;
    // the fold of the launch before, if it is still pending: offered to this launch (launch_phase2_3 takes it into its
    // grid when the kernel has that form), else launched by itself behind it -- before the launch after this one either way
    vl.fin = ctx->pending_fin, vl.fin_cell = ctx->census_pending;
    ctx->pending_fin.nblk = 0;
    const Launched did = launch_phase2(ctx, vl, b, fused, grid);
    if (vl.fin.nblk && !did.took_fin) {
      launch_fin_alone(ctx, vl.fin);
      census_fold(ctx, vl.fin_cell, FPX_CENSUS_FOLD_BEHIND);
    }
    rc = launch_check(ctx);
    if (rc) return rc;
    if (pass == 1 && prof) ctx->ev_used += 2;
    if (b.solo) continue;
    // this launch's own fold: with a ballot per cell no vote kernel reads what it writes -- it waits for the next launch
    // (or for whatever touches the context next); with a round per acceptor the next vote kernel starts from it: at once
    const FinJob fj = fin_job_of(ctx, vl.st, b, grid);
    const bool no_defer = getenv("FPX_NO_DEFER_FINALIZE") != nullptr;  // (read per launch: a test switches it between contexts)
    if (fused && ctx->g.per_slot && !no_defer) {
      ctx->pending_fin = fj;
      ctx->census_pending = did.cell;
    } else {
      census_fold(ctx, did.cell, FPX_CENSUS_FOLD_NOW);
      launch_fin_alone(ctx, fj);
      rc = launch_check(ctx);
      if (rc) return rc;
    }
  }
  return FPX_OK;
}

int enqueue_open(fpx_ctx* ctx, Batch& b, const RunOpts& opts) {
  if (b.n == 0) return FPX_OK;
  int rc = enqueue_validate(ctx, b, false, opts);
  if (rc) return rc;
  hipLaunchKernelGGL(k_open, dim3((b.n + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, b);
  return launch_check(ctx);
}

int enqueue_tally(fpx_ctx* ctx, Batch& b, const RunOpts& opts) {
  if (b.n == 0) return FPX_OK;
  int rc = enqueue_validate(ctx, b, false, opts);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tally, dim3((b.n + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, b);
  return launch_check(ctx);
}

// ---- one device run, as the _dev entry points and the host-pointer paths launch it -----------------------------------
// An exported _dev function is the device guard, the argument check and an enqueue_* / run_* with RunOpts{}; a host-pointer
// path calls the same with the RunOpts of its run.  None of them touches a pending fold on its way in: enqueue_phase2 offers
// it to its launch, the callers of the others launch it first (DeviceGuard, or flush_pending_fin by hand).
Batch batch_of(int32_t n, const int32_t* d_slot, const int32_t* d_round, const int32_t* d_value_id,
               const uint64_t* d_target_mask = nullptr) {
  Batch b;
  memset(&b, 0, sizeof(b));
  b.n = n, b.slot = d_slot, b.round = d_round, b.value = d_value_id, b.target = d_target_mask;
  return b;
}

// messages [lo, lo + len) of a batch whose arrays are staged whole (a run of a host batch)
Batch run_of(const Batch& w, int lo, int len) {
  const auto at = [lo](auto* p, size_t per) { return p ? p + (size_t)lo * per : p; };
  Batch b = w;
  b.n = len, b.slot = at(w.slot, 1), b.round = at(w.round, 1), b.value = at(w.value, 1), b.target = at(w.target, 4);
  b.vote_bits = at(w.vote_bits, 4), b.nack_bits = at(w.nack_bits, 4), b.nack_round = at(w.nack_round, 1);
  b.chosen = at(w.chosen, 1), b.chosen_round = at(w.chosen_round, 1), b.chosen_value = at(w.chosen_value, 1);
  b.is_new = at(w.is_new, 1);
  return b;
}

int run_phase2_fused(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round, const int32_t* d_value_id,
                     const uint64_t* d_target_mask, uint8_t* d_chosen, int32_t* d_chosen_round, int32_t* d_chosen_value,
                     int32_t* d_nack_round, const RunOpts& opts) {
  Batch b = batch_of(n, d_slot, d_round, d_value_id, d_target_mask);
  b.chosen = d_chosen, b.chosen_round = d_chosen_round, b.chosen_value = d_chosen_value, b.nack_round = d_nack_round;
  return enqueue_phase2(ctx, b, true, opts);
}

int run_replica_chosen(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_value_id, const uint8_t* d_mask,
                       const RunOpts& opts) {
  if (n == 0) return FPX_OK;
  Batch b = batch_of(n, d_slot, nullptr, d_value_id);
  b.mask = d_mask;
  int rc = enqueue_validate(ctx, b, false, opts);
  if (rc) return rc;
  const int ingest_grid = std::max(1, std::min({(n + 255) / 256, ctx->num_cus * 8, LG_MAX_PARTS}));
  hipLaunchKernelGGL(k_log_ingest, dim3(ingest_grid), dim3(256), 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_log_prep, dim3(1), dim3(256), 0, ctx->stream, ctx->g, ctx->st, ingest_grid);
  hipLaunchKernelGGL(k_log_scan, dim3(ctx->num_cus * 4), dim3(256), 0, ctx->stream, ctx->g, ctx->st);
  hipLaunchKernelGGL(k_log_commit, dim3(1), dim3(1), 0, ctx->stream, ctx->st);
  return launch_check(ctx);
}

// the owner table, the messages' entries and the gathered rows (zeroed) of a claim / gather / tally call
int prepare_tally_msgs(fpx_ctx* ctx, MsgBatch& b) {
  int rc;
  if ((rc = claim_array(ctx, &ctx->m_owner, (size_t)ctx->g.S * ctx->g.wp))) return rc;
  if ((rc = grow(ctx, &ctx->m_entry, (size_t)b.n * 4))) return rc;
  if ((rc = grow(ctx, &ctx->m_rows, (size_t)b.n * 32))) return rc;
  b.owner = (int32_t*)ctx->m_owner.p, b.entry = (int32_t*)ctx->m_entry.p, b.row_bits = (unsigned long long*)ctx->m_rows.p;
  b.phase2b = FPX_WIRE_PHASE2B;
  HIPCHK(ctx, hipMemsetAsync(b.row_bits, 0, (size_t)b.n * 32, ctx->stream));
  return FPX_OK;
}

// ProxyLeader.handlePhase2b for per-acceptor messages: claim, gather, tally, tail (fpx_tally_msgs.hpp)
int enqueue_tally_msgs(fpx_ctx* ctx, MsgBatch& b) {
  if (b.n == 0) return FPX_OK;
  int rc = prepare_tally_msgs(ctx, b);
  if (rc) return rc;
  const dim3 grid((b.n + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_msgs_claim, grid, blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_msgs_gather, grid, blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_msgs_tally, grid, blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_msgs_tail, dim3(1), dim3(1), 0, ctx->stream, ctx->st, b);
  return launch_check(ctx);
}

// fetch + clear the sticky device status (synchronises the stream)
int fetch_status(fpx_ctx* ctx) {
  int32_t h[4] = {0, 0, 0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h, ctx->st.status, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (h[0] != 0) {
    ctx->err_index = h[ST_INDEX];
    ctx->err_slot = h[ST_SLOT];
    ctx->err_round = h[ST_ROUND];
    HIPCHK(ctx, hipMemsetAsync(ctx->st.status, 0, sizeof(int32_t) * 8, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return h[0];
}

int clear_range_table(fpx_ctx* ctx, const RangeTable& t) {
  if (!t.key) return FPX_OK;
  const size_t words = (size_t)ctx->g.num_groups * 4;
  HIPCHK(ctx, hipMemsetAsync(t.key, 0, (size_t)t.cap * 16, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(t.bits, 0, (size_t)t.cap * words * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(t.owner, 0x7F, (size_t)t.cap * 4, ctx->stream));  // 0x7f7f7f7f: above any message index
  HIPCHK(ctx, hipMemsetAsync(t.count, 0, 4, ctx->stream));
  return FPX_OK;
}

int init_state(fpx_ctx* ctx) {
  const Geom& g = ctx->g;
  State& st = ctx->st;
  const size_t ncell = (size_t)g.S * g.RS, nsc = (size_t)g.ngroups * g.R;
  HIPCHK(ctx, hipMemsetAsync(st.promised, 0xFF, nsc * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.max_voted, 0xFF, nsc * 4, ctx->stream));
  if (g.VS != g.RS) {
    HIPCHK(ctx, hipMemsetAsync(st.vote_round, 0xFF, ncell * 8, ctx->stream));  // both rows of every slot, interleaved
  } else {
    HIPCHK(ctx, hipMemsetAsync(st.vote_round, 0xFF, ncell * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(st.vote_value, 0xFF, ncell * 4, ctx->stream));
  }
  if (st.ballot) HIPCHK(ctx, hipMemsetAsync(st.ballot, 0xFF, ncell * 4, ctx->stream));
  if (st.ballot_sum) HIPCHK(ctx, hipMemsetAsync(st.ballot_sum, 0xFF, (size_t)g.S * 4, ctx->stream));  // every row -1
  HIPCHK(ctx, hipMemsetAsync(st.pl_key, 0, (size_t)g.S * g.wp * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.pl_value, 0xFF, (size_t)g.S * g.wp * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.pl_bits, 0, (size_t)g.S * g.wp * 32, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.stamp, 0, (size_t)g.S * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.row_voted, 0, (size_t)g.S, ctx->stream));  // ROW_FRESH (the records of fresh rows are never read)
  HIPCHK(ctx, hipMemsetAsync(st.lz_round, 0xFF, (nsc + 4) * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.lz_from, 0, (nsc + 4) * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.max_ballot, 0xFF, (nsc + 4) * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.p1, 0, ((size_t)4 * g.R + 64) * 4, ctx->stream));
  ctx->lazy_active = false, ctx->lz_min_from = 0x7fffffff;
  ctx->may_compact = false;
  HIPCHK(ctx, hipMemsetAsync(st.run_round, 0xFF, (size_t)g.ngroups * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.status, 0, 8 * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.part_stamp, 0, (size_t)2 * ctx->max_grid * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.part_all, 0xFF, (size_t)3 * 64 * PART_ALL_STRIDE * 4, ctx->stream));
  ctx->pending_fin.nblk = 0;
  HIPCHK(ctx, hipMemsetAsync(st.log_value, 0xFF, (size_t)g.S * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(st.log_present, 0, (size_t)g.S, ctx->stream));
  for (int k = 0; k < 2; ++k) {
    int rc2 = clear_range_table(ctx, ctx->rt[k]);
    if (rc2) return rc2;
  }
  ctx->rt_cur = 0;
  {
    // executedWatermark = 0, numChosen = 0, largestKey = -1, scan result = 0
    static const int32_t init[8] = {0, 0, -1, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(st.log_scalars, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
  }
  ctx->run_id = 0;
  ctx->hrun = 0;
  std::fill(ctx->hstamp.begin(), ctx->hstamp.end(), 0u);
  return FPX_OK;
}


// ---- chunk placement of the cell slab (round 5; profiles/r05_placement.md) --------------------------------------------
// The hot kernel streams row s of two or three arrays in lockstep: it reads the ballot row and WRITES the two vote rows.
// How fast that goes depends on which physical memory the rows written together sit in: two 1 GiB regions are either
// compatible (written side by side at 6.7 TB/s) or not (5.6 TB/s, the rate of one write stream alone) -- a property of the
// pair's physical addresses, about half of all pairs each way, identical for every repetition; the read stream's region
// matters a few percent more.  One hipMalloc of the whole slab pairs window w of vote_round with window w of vote_value at
// whatever distance the allocation's shape dictates: stretches of windows at the slow rate, stretches at the fast one (the
// "placement lottery" of rounds 1 - 4: 0.535 - 0.607 ms for the same launch).  So the slab is a reserved address range
// backed by 1 GiB physical allocations (hipMemCreate), and WHICH allocation backs which gigabyte of which array is chosen
// by measurement: for every gigabyte of vote_round a partner for vote_value that probes fast (k_probe: the hot access
// pattern on half of the chunk), then the best of a few candidates for the ballots.  The kernels see one contiguous slab.
constexpr size_t PLACE_CHUNK = (size_t)1 << 30;

struct Placer {
  fpx_ctx* ctx;
  char* base = nullptr;
  size_t reserved = 0;
  std::vector<hipMemGenericAllocationHandle_t> h;  // pool; chunk i is mapped at base + i * PLACE_CHUNK while probing
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int q4 = 64, rows = 1 << 19;
  int probes = 0;
  char* at(int i) const { return base + (size_t)i * PLACE_CHUNK; }
  // the hot access pattern on `rows` rows: write chunks b and c (c < 0: one stream), read chunk a (a < 0: none); min of 2
  float probe(int b, int c, int a) {
    float best = 1e30f;
    for (int rep = 0; rep < 2; ++rep) {
      (void)hipEventRecord(e0, ctx->stream);
      hipLaunchKernelGGL(k_probe, dim3((rows + 127) / 128), dim3(256), 0, ctx->stream, a < 0 ? nullptr : (int32_t*)at(a), (int32_t*)at(b),
                         c < 0 ? nullptr : (int32_t*)at(c), rows, q4, 1, (long long)rows);
      (void)hipEventRecord(e1, ctx->stream);
      if (hipEventSynchronize(e1) != hipSuccess) return -1.f;
      float m = 0;
      if (hipEventElapsedTime(&m, e0, e1) != hipSuccess) return -1.f;
      best = std::min(best, m);
    }
    ++probes;
    return best;
  }
  void release_all() {
    if (base) {
      for (size_t i = 0; i < h.size(); ++i) (void)hipMemUnmap((hipDeviceptr_t)at((int)i), PLACE_CHUNK);
    }
    for (auto x : h) (void)hipMemRelease(x);
    h.clear();
    if (base) (void)hipMemAddressFree((hipDeviceptr_t)base, reserved);
    base = nullptr;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
    (void)hipGetLastError();
  }
};

// Builds the slab of `narr` arrays of `array_bytes` each out of chosen chunks.  On success: *slab_out / *stride_out (the
// arrays' distance, a multiple of the chunk), the context owns the reservation and the chunks.  Any failure leaves nothing
// behind and the caller falls back to one hipMalloc.
bool place_chunks(fpx_ctx* ctx, int narr, size_t array_bytes, int q4, char** slab_out, size_t* stride_out) {
  const int per = (int)((array_bytes + PLACE_CHUNK - 1) / PLACE_CHUNK), need = per * narr;
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = ctx->cfg.device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0 || PLACE_CHUNK % gran) {
    (void)hipGetLastError();
    return false;
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  // spare chunks give the search somewhere to go when the pool's mix is lopsided; they are released afterwards
  int spare = std::min(need / 2 + 4, 24);
  while (spare > 0 && free_b < (size_t)(need + spare) * PLACE_CHUNK + ((size_t)8 << 30)) --spare;
  if (free_b < (size_t)need * PLACE_CHUNK + ((size_t)4 << 30)) return false;
  int pool = need + spare;
  Placer P;
  P.ctx = ctx, P.q4 = q4;
  P.rows = (int)std::min<size_t>(PLACE_CHUNK / 2 / ((size_t)q4 * 16), (size_t)1 << 19);
  P.reserved = (size_t)pool * PLACE_CHUNK;
  hipDeviceptr_t va = nullptr;
  if (hipMemAddressReserve(&va, P.reserved, PLACE_CHUNK, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  P.base = (char*)va;
  if (hipEventCreate(&P.e0) != hipSuccess || hipEventCreate(&P.e1) != hipSuccess) {
    P.release_all();
    return false;
  }
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  // The pool grows chunk by chunk.  Other contexts may be created on this device at the same moment (the world-N tests:
  // N ranks probing at once), so the one snapshot above is not trusted for the spares: free memory is asked again every
  // 8 chunks, and the first hipMemCreate that fails -- or free memory under the 4 GiB of headroom -- means "stop growing":
  // with the `need` chunks in hand the search goes on without spares, short of them the caller takes one hipMalloc
  // (the spares must not starve another process's allocation, nor cost the placement itself).
  int got = 0;
  for (int i = 0; i < pool; ++i) {
    if (i >= need && (i & 7) == 0) {
      size_t fb2 = 0, tb2 = 0;
      if (hipMemGetInfo(&fb2, &tb2) != hipSuccess || fb2 < PLACE_CHUNK + ((size_t)8 << 30)) break;
    }
    hipMemGenericAllocationHandle_t hd;
    if (hipMemCreate(&hd, PLACE_CHUNK, &prop, 0) != hipSuccess) {
      (void)hipGetLastError();
      break;
    }
    P.h.push_back(hd);
    if (hipMemMap((hipDeviceptr_t)P.at(i), PLACE_CHUNK, 0, hd, 0) != hipSuccess) {
      P.h.pop_back();
      (void)hipMemRelease(hd);
      (void)hipGetLastError();
      break;
    }
    ++got;
  }
  if (got < need) {
    P.release_all();
    return false;
  }
  pool = got;
  if (hipMemSetAccess((hipDeviceptr_t)P.base, (size_t)pool * PLACE_CHUNK, &acc, 1) != hipSuccess) {
    P.release_all();
    return false;
  }
  const bool dbg = getenv("FPX_DEBUG") != nullptr;
  // The search has a budget in wall-clock milliseconds (FPX_PLACEMENT_BUDGET_MS, default 300; VERDICT r05 weak #8 / next #7:
  // eight ranks probing one node at once must not stretch fpx_create): once it is spent every remaining decision takes its
  // first candidate unprobed -- the slab is then placed as allocated from that window on, which is what one hipMalloc does.
  double budget_ms = 300.0;
  if (const char* e = getenv("FPX_PLACEMENT_BUDGET_MS")) budget_ms = atof(e);
  const auto t_start = std::chrono::steady_clock::now();
  auto over_budget = [&]() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count() > budget_ms;
  };
  int unprobed = 0;
  (void)P.probe(0, narr > 1 ? 1 : -1, -1);  // clocks up, code object loaded
  std::vector<int> freec;                   // chunks not assigned yet, in allocation order
  for (int i = 0; i < pool; ++i) freec.push_back(i);
  std::vector<int> pb(per), pc(per, -1), pa(per, -1);
  float pair_min = 1e30f, tri_min = 1e30f;
  bool bad = false;
  // vote_round's chunk of window w is the next free one; vote_value's the first candidate that probes within 6 % of the
  // fastest pair seen (a slow pair is 18 - 20 % off), else the best of up to 16.  Compatible regions come in stretches of
  // tens of gigabytes, so the candidates are taken SPREAD over the free list (its positions in bit-reversed order: the
  // middle, the quarters, the eighths ..), not from its front -- eight neighbours were eight chunks of one kind and left
  // 6 of 25 windows slow (profiles/r05_placement.md)
  auto spread = [](int k, int nfree) {  // the k-th candidate position among nfree
    int bits = 0;
    while ((1 << bits) < nfree) ++bits;
    for (int i = 0, seen = 0; i < (1 << bits); ++i) {
      int r = 0;
      for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
      if (r < nfree && seen++ == k) return r;
    }
    return k % std::max(1, nfree);
  };
  std::vector<int> aside;  // chunks that found no partner as vote_round's: back into the pool for the ballots / as spares
  for (int w = 0; w < per && !bad; ++w) {
    // up to 4 different chunks for vote_round: late in the search the pool may have run out of partners for the kind of
    // chunk at its front (both other arrays draw from it); such a chunk is set aside and the next one tried
    int fb = -1, fcid = -1;  // the pair so far (chunk ids)
    float ft = 1e30f;
    for (int attempt = 0; attempt < 4 && !bad; ++attempt) {
      // (the windows after this one need two chunks each, and the ballots one per window: ADVICE r05)
      if ((int)freec.size() + (int)aside.size() < 2 + (per - w - 1) * 2 + (narr >= 3 ? per : 0) || freec.size() < 2) break;
      const int b = freec.front();
      freec.erase(freec.begin());
      int best_c = -1;
      float best_t = 1e30f;
      const int nfree = (int)freec.size(), tries = std::min(nfree, 16);
      bool fast = false;
      for (int q = 0; q < tries; ++q) {
        const int c = freec[spread(q, nfree)];
        if (over_budget()) {  // no more probes: the first candidate
          if (best_c < 0) best_c = c, best_t = pair_min < 1e29f ? pair_min : 0.f, ++unprobed;
          fast = true;
          break;
        }
        const float t = P.probe(b, c, -1);
        if (t < 0) { bad = true; break; }
        if (t < best_t) best_t = t, best_c = c;
        pair_min = std::min(pair_min, t);
        if ((w > 0 || q >= 11) && t <= pair_min * 1.06f) { fast = true; break; }  // (window 0 looks at 12 at least: it calibrates pair_min)
      }
      if (bad) break;
      if (w == 0 && best_t <= pair_min * 1.06f) fast = true;
      if (fb < 0 || best_t < ft) {
        if (fb >= 0) aside.push_back(fb);
        fb = b, fcid = best_c, ft = best_t;
      } else {
        aside.push_back(b);
      }
      if (fast) break;
    }
    if (bad || fb < 0 || fcid < 0) { bad = true; break; }
    // the partner is still free: in the pool, or set aside after a turn as vote_round's candidate
    auto take = [&](std::vector<int>& from) {
      auto it = std::find(from.begin(), from.end(), fcid);
      if (it == from.end()) return false;
      from.erase(it);
      return true;
    };
    if (!take(freec) && !take(aside)) { bad = true; break; }
    pb[w] = fb, pc[w] = fcid;
    if (dbg) fprintf(stderr, "libfpx: placement window %d: vote_round chunk %d + vote_value chunk %d: %.4f ms (fastest pair so far %.4f)\n", w, pb[w], pc[w], ft, pair_min);
  }
  freec.insert(freec.end(), aside.begin(), aside.end());
  // the ballots' chunk: the first candidate (spread over what is left, as above) within 1 % of the fastest triple stream
  // seen, else the best of 12.  The read stream's region matters as much as the pair's: with three candidates 3 of 25
  // windows ended 10 % slow, with eight none (profiles/r05_placement.md)
  const int a_tries = 12;
  std::vector<float> win_ms(per, 0.f);
  for (int w = 0; w < per && !bad; ++w) {
    if (narr < 3) {
      win_ms[w] = over_budget() ? (pair_min < 1e29f ? pair_min : 0.f) : P.probe(pb[w], pc[w], -1);
      continue;
    }
    int best_k = -1;
    float best_t = 1e30f;
    const int left = per - w;  // windows that still need a chunk: never look at more candidates than can be spared
    const int na = std::max(1, std::min({(int)freec.size() - (left - 1), a_tries, 16}));
    for (int q = 0; q < na; ++q) {
      const int k = spread(q, (int)freec.size());
      if (over_budget()) {
        if (best_k < 0) best_k = k, best_t = tri_min < 1e29f ? tri_min : 0.f, ++unprobed;
        break;
      }
      const float t = P.probe(pb[w], pc[w], freec[k]);
      if (t < 0) { bad = true; break; }
      if (t < best_t) best_t = t, best_k = k;
      tri_min = std::min(tri_min, t);
      if (w > 0 && t <= tri_min * 1.01f) break;
    }
    if (bad || best_k < 0) { bad = true; break; }
    pa[w] = freec[best_k];
    freec.erase(freec.begin() + best_k);
    win_ms[w] = best_t;
    if (dbg) fprintf(stderr, "libfpx: placement window %d: ballot chunk %d: %.4f ms (fastest triple so far %.4f)\n", w, pa[w], best_t, tri_min);
  }
  if (bad) {
    P.release_all();
    return false;
  }
  // the final order: array 0 = vote_round, 1 = vote_value, 2 = ballot, `per` chunks each; what is left goes back
  std::vector<hipMemGenericAllocationHandle_t> order;
  for (int w = 0; w < per; ++w) order.push_back(P.h[pb[w]]);
  for (int w = 0; w < per; ++w) order.push_back(P.h[pc[w]]);
  if (narr == 3)
    for (int w = 0; w < per; ++w) order.push_back(P.h[pa[w]]);
  for (int i = 0; i < pool; ++i) (void)hipMemUnmap((hipDeviceptr_t)P.at(i), PLACE_CHUNK);
  for (int i : freec) (void)hipMemRelease(P.h[i]);
  P.h = order;
  bool ok = true;
  for (int i = 0; i < need && ok; ++i) ok = hipMemMap((hipDeviceptr_t)P.at(i), PLACE_CHUNK, 0, P.h[i], 0) == hipSuccess;
  ok = ok && hipMemSetAccess((hipDeviceptr_t)P.base, (size_t)need * PLACE_CHUNK, &acc, 1) == hipSuccess;
  if (!ok) {
    P.release_all();
    return false;
  }
  std::vector<float> sorted(win_ms);
  std::sort(sorted.begin(), sorted.end());
  ctx->placement[0] = 1.f, ctx->placement[1] = (float)per, ctx->placement[2] = sorted.front(), ctx->placement[3] = sorted[per / 2],
  ctx->placement[4] = sorted.back();
  if (dbg)
    fprintf(stderr, "libfpx: slab of %d x %d chunks of 1 GiB placed with %d probes in %.0f ms (pool %d, budget %.0f ms, %d decisions unprobed): per-window probe min %.4f median %.4f max %.4f ms\n",
            narr, per, P.probes, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), pool, budget_ms,
            unprobed, sorted.front(), sorted[per / 2], sorted.back());
  ctx->placement_probes = P.probes, ctx->placement_unprobed = unprobed;
  ctx->placement_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  (void)hipEventDestroy(P.e0);
  (void)hipEventDestroy(P.e1);
  ctx->vmm_chunks = P.h;
  ctx->vmm_reserved = P.reserved;
  ctx->slab = P.base;
  *slab_out = P.base;
  *stride_out = (size_t)per * PLACE_CHUNK;
  return true;
}

void free_state(fpx_ctx* ctx) {
  State& st = ctx->st;
  if (ctx->vmm_reserved) {  // the slab is a reservation backed by chunks
    for (size_t i = 0; i < ctx->vmm_chunks.size(); ++i) (void)hipMemUnmap((hipDeviceptr_t)((char*)ctx->slab + i * PLACE_CHUNK), PLACE_CHUNK);
    for (auto h : ctx->vmm_chunks) (void)hipMemRelease(h);
    ctx->vmm_chunks.clear();
    (void)hipMemAddressFree((hipDeviceptr_t)ctx->slab, ctx->vmm_reserved);
    ctx->slab = nullptr, ctx->vmm_reserved = 0;
  }
  void* ps[] = {st.promised, st.max_voted, ctx->slab, st.pl_key, st.pl_value,
                st.pl_bits,  st.stamp,     st.run_round,  st.status,     st.part,
                st.log_value, st.log_present, st.log_scalars, st.part_stamp, st.part_all,
                st.row_voted, st.ballot_sum, st.vote_sum, st.lz_round, st.lz_from, st.max_ballot, st.p1,
                ctx->rt[0].key, ctx->rt[0].bits, ctx->rt[0].owner, ctx->rt[0].count,
                ctx->rt[1].key, ctx->rt[1].bits, ctx->rt[1].owner, ctx->rt[1].count, ctx->d_rng.p, ctx->d_run_done.p};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  free_stage(&ctx->stage);
  DevBuf* bs[] = {&ctx->d_scratch, &ctx->d_enc,   &ctx->m_owner, &ctx->m_entry, &ctx->m_rows,  &ctx->rm_claim,
                  &ctx->rm_buf,    &ctx->mm_claim, &ctx->p1i,     &ctx->p1m_buf, &ctx->p1m_tab, &ctx->ri_buf,
                  &ctx->ai_buf,    &ctx->ai_tkey,  &ctx->ai_tval, &ctx->mai_buf};
  for (DevBuf* b : bs)
    if (b->p) (void)hipFree(b->p);
  for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
  ctx->ev.clear();
  for (hipEvent_t e : ctx->cev) (void)hipEventDestroy(e);
  ctx->cev.clear();
  if (ctx->hslots) {
    for (int k = 0; k < HOST_DEPTH; ++k) {
      HostSlot& h = ctx->hslots[k];
      for (DevBuf& b : h.in)
        if (b.p) (void)hipFree(b.p);
      for (DevBuf& b : h.sink)
        if (b.p) (void)hipFree(b.p);
      if (h.done) (void)hipEventDestroy(h.done);
      if (h.up) (void)hipEventDestroy(h.up);
      if (h.status) (void)hipHostFree(h.status);
    }
    delete[] ctx->hslots;
    ctx->hslots = nullptr;
  }
  if (ctx->band_fork) (void)hipEventDestroy(ctx->band_fork);
  if (ctx->band_join) (void)hipEventDestroy(ctx->band_join);
  if (ctx->band_stream) (void)hipStreamDestroy(ctx->band_stream);
  if (ctx->d_band.p) (void)hipFree(ctx->d_band.p);
  if (ctx->up_stream) (void)hipStreamDestroy(ctx->up_stream);
  if (ctx->d_part.p) (void)hipFree(ctx->d_part.p);
  if (ctx->d_mine.p) (void)hipFree(ctx->d_mine.p);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
}

// ---- host-side run splitting ---------------------------------------------------------------------
// Cuts [0, n) into maximal runs that satisfy the run contract, so that running them back to back
// equals message-at-a-time delivery in array order.
int host_group(const fpx_config& c, int slot) {
  const int lg = slot % c.num_leader_groups;
  const int ag = (slot / c.num_leader_groups) % c.num_groups;
  return lg * c.num_groups + ag;
}

// what check_inputs found about a batch on its way: strictly increasing slots (hence distinct), one round
struct BatchShape { bool increasing = false, one_round = false; };

void split_runs(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round, bool check_round, std::vector<int>* cuts,
                BatchShape shape = {}) {
  cuts->clear();
  cuts->push_back(0);
  // check_inputs saw strictly increasing slots in one round: one run
  if (shape.increasing && (shape.one_round || !check_round || ctx->g.per_slot)) {
    cuts->push_back(n);
    return;
  }
  if (ctx->hstamp.empty()) ctx->hstamp.assign((size_t)ctx->g.S, 0u);
  if (ctx->hround.empty()) ctx->hround.assign((size_t)ctx->g.ngroups, -1);
  check_round = check_round && !ctx->g.per_slot;
  std::vector<int> touched;
  auto new_run = [&]() {
    if (++ctx->hrun == 0) {
      std::fill(ctx->hstamp.begin(), ctx->hstamp.end(), 0u);
      ctx->hrun = 1;
    }
    for (int gidx : touched) ctx->hround[gidx] = -1;
    touched.clear();
  };
  new_run();
  for (int i = 0; i < n; ++i) {
    const int s = slot[i];
    bool cut = ctx->hstamp[s] == ctx->hrun;
    int gidx = 0;
    if (check_round) {
      gidx = ctx->g.ngroups == 1 ? 0 : host_group(ctx->cfg, s);
      if (ctx->hround[gidx] != -1 && ctx->hround[gidx] != round[i]) cut = true;
    }
    if (cut) {
      cuts->push_back(i);
      new_run();
    }
    ctx->hstamp[s] = ctx->hrun;
    if (check_round) {
      if (ctx->hround[gidx] == -1) touched.push_back(gidx);
      ctx->hround[gidx] = round[i];
    }
  }
  cuts->push_back(n);
  for (int gidx : touched) ctx->hround[gidx] = -1;
}

int check_args(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round) {
  return (!ctx || n < 0 || (n > 0 && (!slot || !round))) ? FPX_EINVAL : FPX_OK;
}

// range check of a host batch; the host entry points run it (and split_runs) AFTER enqueueing the uploads,
// so with page-locked buffers (fpx_host_alloc) the CPU passes overlap the DMA.  Nothing is launched on
// a bad batch: the staging copies alone change no protocol state.
int check_inputs(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round, BatchShape* shape = nullptr) {
  // one branch-free pass (vectorises): range of slots and rounds, and whether the batch is the common
  // shape -- strictly increasing slots in one round -- that split_runs can accept as a single run
  int32_t smin = INT32_MAX, smax = INT32_MIN, rmin = INT32_MAX, rmax = INT32_MIN;
  int32_t unordered = 0;
  for (int i = 0; i < n; ++i) {
    smin = std::min(smin, slot[i]), smax = std::max(smax, slot[i]);
    rmin = std::min(rmin, round[i]), rmax = std::max(rmax, round[i]);
  }
  for (int i = 1; i < n; ++i) unordered |= (int32_t)(slot[i] <= slot[i - 1]);
  if (shape) shape->increasing = unordered == 0, shape->one_round = rmin == rmax;  // (of use to a batch in range only)
  if (smin >= 0 && smax < ctx->g.S && rmin >= 0 && rmax <= MAX_ROUND) return FPX_OK;
  for (int i = 0; i < n; ++i) {
    if (slot[i] < 0 || slot[i] >= ctx->g.S || round[i] < 0 || round[i] > MAX_ROUND) {
      ctx->err_index = i;
      ctx->err_slot = slot[i];
      ctx->err_round = round[i];
      break;
    }
  }
  (void)hipStreamSynchronize(ctx->stream);  // the caller's buffers are free again when we return
  return FPX_EINVAL;
}

template <int G>
void launch_p1b(fpx_ctx* ctx, const uint64_t* d_q, int wm, int count, int32_t* d_sr, int32_t* d_sv) {
  const int per_block = 4 * (64 / G);
  const int grid = std::max(1, std::min((count + per_block - 1) / per_block, ctx->num_cus * 16));
  hipLaunchKernelGGL((k_phase1b_scan<G>), dim3(grid), dim3(256), 0, ctx->stream, ctx->g, ctx->st, d_q, wm, count,
                     ctx->vec ? 1 : 0, d_sr, d_sv);
}

// ---- host batches: stage, cut into runs, run, copy back ----------------------------------------------------------
// how a host-pointer call on an fpx_ctx ends: with the device's status (fetch_status synchronises); a held output reaches
// the caller when that is FPX_OK -- the burst was applied
struct CtxEnd {
  fpx_ctx* ctx;
  int operator()() const { return fetch_status(ctx); }
  static bool applied(int rc) { return rc == FPX_OK; }
};

// The launches of a host batch whose arrays are staged.  cut(&cuts) checks the batch on the host -- behind the uploads, so
// with page-locked arrays the CPU pass overlaps the DMA; nothing is launched on a bad batch -- and cuts it into runs that
// satisfy the run contract; run(lo, len, opts) launches messages [lo, lo + len) with opts.index_base = lo (a run addresses
// its slice of a staged array as slot + lo), the runs back to back (= message-at-a-time delivery in array order).
// cut == nullptr: the whole batch is ONE run, validated on the device (RunOpts::FORCE_VALIDATE; the runs of a cut batch
// are RunOpts::CUT_ON_HOST).  A run that fails ends the call: the stream is synchronised, nothing is downloaded.
template <typename Cut, typename Run>
int launch_runs(fpx_ctx* ctx, int n, Cut cut, Run run) {
  constexpr bool cut_on_host = !std::is_null_pointer<Cut>::value;
  int rc;
  std::vector<int> cuts{0, n};
  if constexpr (cut_on_host) {
    if ((rc = cut(&cuts))) return rc;
  }
  RunOpts opts;
  opts.validate = cut_on_host ? RunOpts::CUT_ON_HOST : RunOpts::FORCE_VALIDATE;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    opts.index_base = cuts[k];
    if ((rc = run(cuts[k], cuts[k + 1] - cuts[k], opts))) {
      (void)hipStreamSynchronize(ctx->stream);
      return rc;
    }
  }
  return FPX_OK;
}

// The driver of the host-pointer entry points: host_call (fpx_host.hpp) stages the arrays, the runs are launched, the
// outputs come down -- whatever the device's status says afterwards -- and the device's status is returned.
template <typename Cut, typename Run>
int host_runs(fpx_ctx* ctx, int n, std::initializer_list<Staged> arrays, Cut cut, Run run) {
  return host_call(ctx, arrays, [&] { return launch_runs(ctx, n, cut, run); }, CtxEnd{ctx});
}

// the cuts of a host batch of messages: the range check (the first offender for fpx_error_detail), then split_runs
auto message_runs(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round, bool check_round) {
  return [=](std::vector<int>* cuts) {
    BatchShape shape;
    const int rc = check_inputs(ctx, n, slot, round, &shape);
    if (rc == FPX_OK) split_runs(ctx, n, slot, round, check_round, cuts, shape);
    return rc;
  };
}

// ---- page-locked host batches (fpx_phase2_fused_submit / _wait) ------------------------------------------------------
// A call moves 12 B per slot up (slot, round, value) and 9 - 13 B per slot down (Chosen records, Nack rounds).  How, was
// decided by measuring what each way of crossing PCIe costs the vote kernel it runs beside (profiles/r06_host_path.md,
// microbench/r06_pcie_beside_vote.py; 2^20 x 256 step, vote kernel alone 0.546 ms):
//   inputs by the copy engine on a stream of its own (hipMemcpyAsync, 51 GB/s, 3 x 82 us)             + 3 %
//   inputs read by the vote kernel straight from the mapped arrays                                    + 12 %
//   inputs copied by WORKGROUPS (a staging kernel beside the vote kernel: rounds 2 - 5; or workgroups of the vote
//     kernel's own grid)                                                       + 14 % ... + 50 % with the requests in flight
//   records written by the vote kernel straight into the mapped arrays (posted writes)               + 3 %
//   records copied by workgroups                                                                      + 30 %
// (a shader's reads of host memory hold entries of the L2's fabric queues for microseconds each and the vote kernel's HBM
// requests queue behind them; the copy engine does not go through the L2.)  So: the inputs go up by the copy engine on
// `up_stream` into staging buffers in HBM, validation and the fused step run on the context's stream behind ONE event,
// and the vote kernel's output arrays ARE the caller's page-locked arrays -- no copy down, no third stream, no staging
// kernel.  The status words of the call are snapshotted into page-locked words by a one-wavefront kernel behind the step.
// Every array must be mapped host memory (FPX_EINVAL otherwise).

// the device address of mapped (page-locked) host memory, nullptr for anything else
void* mapped_host(const void* p) {
  if (!p) return nullptr;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: "invalid value", not an error of ours
    return nullptr;
  }
  return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}

int host_submit(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                const uint64_t* target_mask, uint8_t* chosen, int32_t* chosen_round, int32_t* chosen_value,
                int32_t* nack_round, int* ticket) {
  const void* in[4] = {slot, round, value_id, target_mask};
  void* out[4] = {chosen, chosen_round, chosen_value, nack_round};
  void* dout[4];
  for (int a = 0; a < 4; ++a) {
    dout[a] = mapped_host(out[a]);
    if ((in[a] && !mapped_host(in[a])) || (out[a] && !dout[a])) return FPX_EINVAL;
  }
  if (!ctx->hslots) {
    ctx->hslots = new (std::nothrow) HostSlot[HOST_DEPTH];
    if (!ctx->hslots) return FPX_ENOMEM;
  }
  int t = -1;
  for (int k = 0; k < HOST_DEPTH && t < 0; ++k)
    if (!ctx->hslots[(ctx->hnext + k) % HOST_DEPTH].busy) t = (ctx->hnext + k) % HOST_DEPTH;
  if (t < 0) return FPX_ECAPACITY;  // HOST_DEPTH calls in flight: wait for the oldest first
  HostSlot& h = ctx->hslots[t];
  if (!h.up) {
    HIPCHK(ctx, hipEventCreateWithFlags(&h.up, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&h.done, hipEventDisableTiming));
    HIPCHK(ctx, hipHostMalloc((void**)&h.status, 64, hipHostMallocDefault));
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&h.status_dev, h.status, 0));
  }
  if (!ctx->up_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
  const size_t in_elem[4] = {4, 4, 4, 32};
  int rc;
  for (int a = 0; a < 4; ++a)
    if (in[a] && (rc = grow(ctx, &h.in[a], (size_t)n * in_elem[a]))) return rc;
  const size_t out_elem[3] = {1, 4, 4};
  for (int a = 0; a < 3; ++a)
    if (!dout[a]) {  // (nack_round alone may be null for the vote kernel)
      if ((rc = grow(ctx, &h.sink[a], (size_t)n * out_elem[a]))) return rc;
      dout[a] = h.sink[a].p;
    }
  for (int a = 0; a < 4; ++a)
    if (in[a]) HIPCHK(ctx, hipMemcpyAsync(h.in[a].p, in[a], (size_t)n * in_elem[a], hipMemcpyHostToDevice, ctx->up_stream));
  HIPCHK(ctx, hipEventRecord(h.up, ctx->up_stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, h.up, 0));
  // one run, validated on the device; a fold that the caller's guard left pending rides in its launch
  rc = run_phase2_fused(ctx, n, (int32_t*)h.in[0].p, (int32_t*)h.in[1].p, (int32_t*)h.in[2].p,
                        target_mask ? (uint64_t*)h.in[3].p : nullptr, (uint8_t*)dout[0], (int32_t*)dout[1], (int32_t*)dout[2],
                        (int32_t*)dout[3], RunOpts{RunOpts::FORCE_VALIDATE});
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  hipLaunchKernelGGL(k_status_snap, dim3(1), dim3(64), 0, ctx->stream, ctx->st.status, h.status_dev);
  HIPCHK(ctx, hipEventRecord(h.done, ctx->stream));
  if ((rc = launch_check(ctx))) return rc;
  h.busy = true, h.n = n;
  ctx->hnext = (t + 1) % HOST_DEPTH;
  *ticket = t;
  return FPX_OK;
}

// the status of call `ticket` as the device left it right after that call's fused step (a run-contract violation or a
// range error aborts the call -- and the calls queued behind it -- before anything is applied)
int host_wait(fpx_ctx* ctx, int ticket) {
  if (!ctx->hslots || ticket < 0 || ticket >= HOST_DEPTH || !ctx->hslots[ticket].busy) return FPX_EINVAL;
  HostSlot& h = ctx->hslots[ticket];
  const hipError_t e = hipEventSynchronize(h.done);
  h.busy = false;
  if (e != hipSuccess) {
    ctx->last_hip = (int)e;
    return FPX_EHIP;
  }
  const int st = h.status[0];
  if (st != 0) {
    // drain and clear the sticky status (the calls behind this one have aborted too and report it from their own copy)
    const int now = fetch_status(ctx);
    if (now == 0) ctx->err_index = h.status[ST_INDEX], ctx->err_slot = h.status[ST_SLOT], ctx->err_round = h.status[ST_ROUND];
  }
  return st;
}

// the synchronous call on page-locked arrays = submit + wait; *used = false: not every array is mapped host memory (or
// calls are in flight) -- the caller takes the copy-engine path
int host_fused_staged(fpx_ctx* ctx, int n, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                      const uint64_t* target_mask, uint8_t* chosen, int32_t* chosen_round, int32_t* chosen_value,
                      int32_t* nack_round, bool* used) {
  *used = false;
  int ticket = -1;
  int rc = host_submit(ctx, n, slot, round, value_id, target_mask, chosen, chosen_round, chosen_value, nack_round, &ticket);
  if (rc == FPX_EINVAL || rc == FPX_ECAPACITY) return FPX_OK;  // not page-locked / ring busy: the other path
  *used = true;
  if (rc) return rc;
  rc = host_wait(ctx, ticket);
  if (rc == FPX_EINVAL) return check_inputs(ctx, n, slot, round);  // the FIRST offender, for fpx_error_detail
  if (rc != FPX_EORDER) return rc;
  // not one device run: cut into runs on the host and replayed (from the copy-engine path's staging buffers)
  *used = false;
  return FPX_OK;
}

// ---- Phase1b.info of every selected acceptor in one pass (fpx_phase1_info.hpp) ------------------------------------
template <int G>
void launch_p1i(fpx_ctx* ctx, const P1iArgs& a, int grid) {
  hipLaunchKernelGGL((k_p1i_count<G>), dim3(grid), dim3(256), 0, ctx->stream, ctx->g, ctx->st, a);
  hipLaunchKernelGGL(k_p1i_colscan, dim3((a.ES + P1I_COLS - 1) / P1I_COLS), dim3(P1I_COLS * P1I_SEGS), 0, ctx->stream, ctx->st, a);
  hipLaunchKernelGGL(k_p1i_offsets, dim3(1), dim3(1024), 0, ctx->stream, ctx->g, ctx->st, a);
  // the scatter: one wavefront per workgroup and (chunk, group, block of 64 acceptors), three workgroups' LDS to a CU
  const int64_t units = (int64_t)a.nchunks * ctx->g.ngroups * (G < 16 ? 1 : G / 16);
  const int sgrid = (int)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)ctx->num_cus * 12));
  hipLaunchKernelGGL((k_p1i_scatter<G>), dim3(sgrid), dim3(64), 0, ctx->stream, ctx->g, ctx->st, a);
}

bool p1i_args_ok(const fpx_ctx* ctx, int64_t cap, const int64_t* offsets, const int32_t* slot, const int32_t* vote_round,
                        const int32_t* vote_value, const int64_t* totals) {
  return ctx && cap >= 0 && offsets && totals && (cap == 0 || (slot && vote_round && vote_value));
}

int enqueue_p1i(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* d_masks, int64_t cap, int64_t* d_offsets,
                       int32_t* d_slot, int32_t* d_vote_round, int32_t* d_vote_value, int64_t* d_totals) {
  const Geom& g = ctx->g;
  P1iArgs a;
  memset(&a, 0, sizeof(a));
  a.masks = d_masks;
  a.lo = chosen_watermark < 0 ? 0 : chosen_watermark;
  a.vec = ctx->vec ? 1 : 0;
  const int64_t span = (int64_t)P1I_TILE * g.ngroups;
  a.ntiles = (int32_t)((g.S + span - 1) / span);
  a.nchunks = (a.ntiles + P1I_CHUNK - 1) / P1I_CHUNK;
  a.ES = g.ngroups * g.RS;
  int rc;
  if ((rc = grow(ctx, &ctx->p1i, ((size_t)a.nchunks * a.ES + a.ES + 4) * 4))) return rc;
  a.csum = (int32_t*)ctx->p1i.p;
  a.ctot = a.csum + (size_t)a.nchunks * a.ES;
  a.go = a.ctot + a.ES;
  a.cap = cap;
  a.offsets = d_offsets, a.slot = d_slot, a.vote_round = d_vote_round, a.vote_value = d_vote_value, a.totals = d_totals;
  // one wavefront per (chunk, group), four to a workgroup, grid-stride beyond num_cus * 8 workgroups
  const int64_t units = (int64_t)a.nchunks * g.ngroups;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((units + 3) / 4, (int64_t)ctx->num_cus * 8));
  switch (ctx->lanes_per_slot) {
    case 1: launch_p1i<1>(ctx, a, grid); break;
    case 2: launch_p1i<2>(ctx, a, grid); break;
    case 4: launch_p1i<4>(ctx, a, grid); break;
    case 8: launch_p1i<8>(ctx, a, grid); break;
    case 16: launch_p1i<16>(ctx, a, grid); break;
    case 32: launch_p1i<32>(ctx, a, grid); break;
    default: launch_p1i<64>(ctx, a, grid); break;
  }
  return launch_check(ctx);
}

// the host form's staging: the masks up (`masks`; or they are on the device already, `d_masks`; neither: every acceptor),
// offsets / records / totals down -- ONE run of the staging driver
int host_p1i(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* masks, const uint64_t* d_masks, int64_t cap,
             int64_t* offsets, int32_t* slot, int32_t* vote_round, int32_t* vote_value, int64_t* count) {
  const size_t E = (size_t)ctx->g.ngroups * ctx->g.R;
  int64_t totals[2] = {0, 0};
  uint64_t* d_up;
  int64_t *d_off, *d_tot;
  int32_t *d_slot, *d_vr, *d_vv;
  const int rc = host_runs(ctx, 1,
                           {opt_in(d_up, masks, (size_t)ctx->g.ngroups * 4), out(d_off, offsets, E + 1), out(d_slot, slot, cap),
                            out(d_vr, vote_round, cap), out(d_vv, vote_value, cap), out(d_tot, totals, 2)},
                           nullptr, [&](int, int, const RunOpts&) {
                             return enqueue_p1i(ctx, chosen_watermark, masks ? d_up : d_masks, cap, d_off, d_slot, d_vr, d_vv, d_tot);
                           });
  if (count) *count = totals[0];
  return rc;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
// ---- the wire adapter on the device (include/fpx_wire.h) ---------------------------------------------------
template <int WHICH>
static int32_t wire_decode_dev(fpx_ctx* ctx, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_offsets, int32_t n,
                               const WireOut& o) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30) || buf_len < 0) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!d_buf || !d_offsets || !o.kind || !o.slot || !o.round) return FPX_EINVAL;
  hipLaunchKernelGGL(k_wire_decode<WHICH>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st, d_buf, buf_len,
                     d_offsets, n, o);
  hipLaunchKernelGGL(k_wire_tail, dim3(1), dim3(1), 0, ctx->stream, ctx->st);
  HIPCHK(ctx, hipGetLastError());
  return FPX_OK;
}


// ---- the device encoders (fpx_wire_enc_dev.hpp) -----------------------------------------------------------------
template <int KIND>
static int32_t wire_encode_dev(fpx_ctx* ctx, EncArgs a) {
  a.nblk = (a.n + ENC_BLOCK - 1) / ENC_BLOCK;
  int rc = grow(ctx, &ctx->d_enc, (size_t)(ENC_W_SUMS + 2 * (size_t)a.nblk) * 8);
  if (rc) return rc;
  a.scratch = (int64_t*)ctx->d_enc.p;
  if (a.nblk) {
    HIPCHK(ctx, hipMemsetAsync(a.scratch, 0x7f, 8, ctx->stream));  // ENC_NO_BAD
    hipLaunchKernelGGL(k_enc_len<KIND>, dim3(a.nblk), dim3(ENC_BLOCK), 0, ctx->stream, a);
  }
  hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(1024), 0, ctx->stream, ctx->st, a);
  if (a.nblk) {
    if (KIND == ENC_PHASE2B) hipLaunchKernelGGL(k_enc_emit_p2b, dim3(a.nblk), dim3(ENC_BLOCK), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_enc_emit_hv<KIND>, dim3(a.nblk), dim3(ENC_BLOCK), 0, ctx->stream, a);
  }
  return launch_check(ctx);
}

static bool enc_common_ok(const fpx_ctx* ctx, int32_t n, const uint8_t* d_out, int64_t cap, const int64_t* d_out_offsets,
                          int64_t max_msgs, const int64_t* d_totals) {
  return ctx && n >= 0 && n < (1 << 30) && cap >= 0 && max_msgs >= 0 && d_out_offsets && d_totals && (d_out || cap == 0);
}

extern "C" {

int32_t fpx_version(void) { return FPX_VERSION; }

const char* fpx_strerror(int32_t s) {
  switch (s) {
    case FPX_OK: return "ok";
    case FPX_EINVAL: return "invalid argument (require failed)";
    case FPX_EFATAL_UNKNOWN_SLOTROUND: return "Phase2b for a (slot, round) that was never opened (logger.fatal)";
    case FPX_EHIP: return "HIP runtime error";
    case FPX_ENODEVICE: return "no usable gfx950 device (libfpx has no CPU fallback)";
    case FPX_ECAPACITY: return "more live (slot, round) tallies for one slot than tally_ways";
    case FPX_EORDER: return "device batch violates the run contract; nothing was applied";
    case FPX_ENOMEM: return "out of device memory";
    case FPX_ERCCL: return "RCCL error (or RCCL could not be loaded)";
    case FPX_EFATAL_PROTOCOL: return "a logger.fatal / logger.check of the reference would have fired; the message was skipped";
    default: return "unknown status";
  }
}

int32_t fpx_config_check(const fpx_config* cfg) { return check_config(cfg); }

int32_t fpx_round_leader(int32_t n, int32_t round) { return round % n; }

int32_t fpx_next_classic_round(int32_t n, int32_t leader_index, int32_t round) {
  if (round < 0) return leader_index;
  const int32_t smallest_multiple = n * (round / n);
  const int32_t offset = leader_index % n;
  return smallest_multiple + offset > round ? smallest_multiple + offset : smallest_multiple + n + offset;
}

int32_t fpx_create(const fpx_config* cfg, fpx_ctx** out) {
  if (!out) return FPX_EINVAL;
  *out = nullptr;
  int rc = check_config(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
    return FPX_ENODEVICE;
  fpx_ctx* ctx = new (std::nothrow) fpx_ctx();
  if (!ctx) return FPX_ENOMEM;
  ctx->cfg = *cfg;
  if (!ctx->cfg.replicas_total) ctx->cfg.replicas_total = cfg->num_replicas;
  make_geom(ctx->cfg, &ctx->g);
  memset(&ctx->st, 0, sizeof(ctx->st));
  memset(ctx->rt, 0, sizeof(ctx->rt));
  DeviceGuard _dg(cfg->device);  // the caller's current device is restored on every return path
  if (hipSetDevice(cfg->device) != hipSuccess) {
    delete ctx;
    return FPX_ENODEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
  // 32 workgroups per CU: at 2^20 messages every wavefront gets exactly one CHUNK-message chunk and
  // the hardware dispatcher load-balances them (measured r01: +10 % over a 2048-workgroup persistent
  // grid, a further +8 % going from 64- to 32-message chunks).  Where vote-row records are written (chunk_for:
  // CHUNK_RECORDS = 64 messages) the same 2^20 messages are half as many workgroups, 16 per CU, still one chunk each
  int G = 1;
  while (G * 4 < ctx->g.R) G <<= 1;
  ctx->lanes_per_slot = G;
  // small groups (R <= 16, the reference's everyday f = 1..3): a 64-slot chunk is three dependent round
  // trips and a workgroup's fixed costs (LDS tables, the final reduction) dominate -- 4 workgroups per CU,
  // each wave walking many chunks, measured 2x faster at R = 3 (profiles/r01_small_r.txt).  Six per CU is what the kernel's
  // LDS (23.5 KB with the column-quad staging) lets be resident at once: 3 - 4 % faster than four on BASELINE.json configs[4],
  // 5 - 15 % on configs[2]; seven and more (a second round of workgroups) are 8 % slower (profiles/r05_cfg5.md)
  ctx->max_grid = ctx->num_cus * (G <= 4 ? 6 : 32);
  ctx->vec = true;  // rows are padded to a multiple of 4 cells (Geom::RS)
  // big tables: fewer resident blocks so that the partial table stays small
  const int ntab = ctx->g.ngroups * ctx->g.R;
  if (ntab > 1024) ctx->max_grid = std::max(ctx->num_cus, ctx->max_grid * 1024 / ntab);

  auto fail = [&](int code) {
    free_state(ctx);
    delete ctx;
    return code;
  };
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(FPX_EHIP);
  ctx->stream = ctx->own_stream;
  const Geom& g = ctx->g;
  State& st = ctx->st;
  const size_t ncell = (size_t)g.S * g.RS, nsc = (size_t)g.ngroups * g.R;
  if ((rc = dalloc(ctx, &st.promised, nsc))) return fail(rc);
  if ((rc = dalloc(ctx, &st.max_voted, nsc))) return fail(rc);
  {
    // the 2-3 cell arrays are streamed in lockstep (row s of each at the same time): one slab (offsets of 1 KiB to 8 MiB
    // between the arrays measured no gain, profiles/r01_stagger_box{A,B}.txt)
    const int narr = g.per_slot ? 3 : 2;
    size_t stride = ncell * 4;
    // Placement: the very same kernel streams a slab at one of two speeds ~7 % apart depending on where the
    // allocation landed (deterministic per allocation, profiles/r02_placement.txt).  A big context therefore
    // allocates up to 4 slabs (while free HBM allows), times the hot access pattern on each (k_probe, 3 x 0.5 ms)
    // and keeps the fastest; the others are freed before anything else is allocated.
    int tries = stride * narr >= ((size_t)2 << 30) && g.RS >= 64 ? 4 : 1;
    char* slab = nullptr;
    // round 5: chunk placement first (place_chunks above) -- a big slab of separate arrays is built from 1 GiB physical
    // chunks paired by measurement; one hipMalloc with candidate probing (rounds 2 - 4) stays the fallback
    bool chunked = false;
    if (tries > 1 && g.VS == g.RS && !(getenv("FPX_PLACEMENT_CHUNKS") && atoi(getenv("FPX_PLACEMENT_CHUNKS")) == 0)) {
      size_t cstride = 0;
      if (place_chunks(ctx, narr, ncell * 4, g.RS / 4, &slab, &cstride)) chunked = true, stride = cstride, tries = 0;
    }
    float best_ms = 0;
    std::vector<char*> losers;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (tries > 1 && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) tries = 1;
    for (int t = 0; t < tries; ++t) {
      if (t > 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < stride * narr + ((size_t)8 << 30)) break;
      }
      char* cand = nullptr;
      if (hipMalloc((void**)&cand, stride * narr) != hipSuccess) {
        (void)hipGetLastError();
        break;
      }
      float ms = 0;
      if (tries > 1) {
        // 2^20 rows in 16 runs spread evenly over the whole slab: placement quality varies WITHIN an allocation too
        const int pieces = g.S >= (1 << 22) ? 16 : 1;
        const int rows = (int)std::min<int64_t>(g.S, 1 << 20) / pieces * pieces, q4 = g.RS / 4;
        const long long piece_stride = g.S / pieces;
        const int grid = (rows + 127) / 128;
        int32_t* a = g.per_slot ? (int32_t*)(cand + 2 * stride) : nullptr;
        float tmin = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {
          (void)hipEventRecord(e0, ctx->stream);
          hipLaunchKernelGGL(k_probe, dim3(grid), dim3(256), 0, ctx->stream, a, (int32_t*)cand, (int32_t*)(cand + stride), rows, q4, pieces, piece_stride);
          (void)hipEventRecord(e1, ctx->stream);
          (void)hipEventSynchronize(e1);
          float m = 0;
          if (hipEventElapsedTime(&m, e0, e1) == hipSuccess && rep > 0) tmin = std::min(tmin, m);
        }
        ms = tmin;
        if (getenv("FPX_DEBUG")) fprintf(stderr, "libfpx: slab placement %d at %p: probe %.4f ms\n", t, (void*)cand, ms);
      }
      if (!slab || ms < best_ms) {
        if (slab) losers.push_back(slab);
        slab = cand, best_ms = ms;
      } else {
        losers.push_back(cand);
      }
    }
    for (char* l : losers) (void)hipFree(l);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (!slab) return fail(FPX_ENOMEM);
    if (!chunked) ctx->placement[0] = 0.f, ctx->placement[1] = 1.f, ctx->placement[2] = ctx->placement[3] = ctx->placement[4] = best_ms;
    ctx->bytes += (int64_t)(stride * narr);
    ctx->slab = slab;
    st.vote_round = (int32_t*)slab;
    st.vote_value = g.VS != g.RS ? st.vote_round + g.RS : (int32_t*)(slab + stride);  // interleaved: the slab's first two
                                                                                      // arrays are one [S][2][RS] array
    st.ballot = g.per_slot ? (int32_t*)(slab + 2 * stride) : nullptr;
  }
  if ((rc = dalloc(ctx, &st.pl_key, (size_t)g.S * g.wp))) return fail(rc);
  if ((rc = dalloc(ctx, &st.pl_value, (size_t)g.S * g.wp))) return fail(rc);
  if ((rc = dalloc(ctx, &st.pl_bits, (size_t)g.S * g.wp * 4))) return fail(rc);
  if ((rc = dalloc(ctx, &st.stamp, (size_t)g.S))) return fail(rc);
  if ((rc = dalloc(ctx, &st.row_voted, (size_t)g.S))) return fail(rc);
  if (g.per_slot && sums_kept(g) && (rc = dalloc(ctx, &st.ballot_sum, (size_t)g.S))) return fail(rc);  // (outside the placed slab)
  if ((rc = dalloc(ctx, &st.lz_round, nsc + 4))) return fail(rc);
  if ((rc = dalloc(ctx, &st.lz_from, nsc + 4))) return fail(rc);
  if ((rc = dalloc(ctx, &st.max_ballot, nsc + 4))) return fail(rc);
  if ((rc = dalloc(ctx, &st.p1, (size_t)4 * g.R + 64))) return fail(rc);
  if ((rc = dalloc(ctx, &st.run_round, (size_t)g.ngroups))) return fail(rc);
  if ((rc = dalloc(ctx, &st.status, (size_t)8))) return fail(rc);
  ctx->g.part_rows = ctx->max_grid;
  // (two halves of the partial rows and their stamps, three thirds of the whole-group shards: finalize_body / k_phase2_fin)
  if ((rc = dalloc(ctx, &st.part, (size_t)2 * ctx->max_grid * 2 * ntab))) return fail(rc);
  if ((rc = dalloc(ctx, &st.part_stamp, (size_t)2 * ctx->max_grid))) return fail(rc);
  if ((rc = dalloc(ctx, &st.part_all, (size_t)3 * 64 * PART_ALL_STRIDE))) return fail(rc);
  if ((rc = dalloc(ctx, &st.log_value, (size_t)g.S))) return fail(rc);
  if ((rc = dalloc(ctx, &st.log_present, (size_t)g.S))) return fail(rc);
  if ((rc = dalloc(ctx, &st.log_scalars, (size_t)LG_PARTS_AT + 2 * LG_MAX_PARTS))) return fail(rc);
  if (!g.per_slot) {
    // noop-range tallies: at most cap / 2 live entries; sized for a few hundred ranges in flight per leader group,
    // bounded to 64 MiB of vote bitmaps per buffer (A x 32 B per entry)
    int64_t want = std::max<int64_t>(4096, (int64_t)g.num_leader_groups * 64);
    const int64_t by_mem = std::max<int64_t>(1024, ((int64_t)64 << 20) / ((int64_t)g.num_groups * 32));
    want = std::min<int64_t>(std::min<int64_t>(want, by_mem), 1 << 18);
    int cap = 1024;
    while (cap < want) cap <<= 1;
    for (int k = 0; k < 2; ++k) {
      RangeTable& t = ctx->rt[k];
      t.cap = cap;
      if ((rc = dalloc(ctx, &t.key, (size_t)cap * 2))) return fail(rc);
      if ((rc = dalloc(ctx, &t.bits, (size_t)cap * g.num_groups * 4))) return fail(rc);
      if ((rc = dalloc(ctx, &t.owner, (size_t)cap))) return fail(rc);
      if ((rc = dalloc(ctx, &t.count, (size_t)1))) return fail(rc);
    }
  }
  // the vote-row records live where the summaries do.  Allocated LAST: every other array of the context then lands
  // where it did before there were records
  if (g.per_slot && sums_kept(g) && (rc = dalloc(ctx, &st.vote_sum, (size_t)g.S))) return fail(rc);
  if ((rc = init_state(ctx))) return fail(rc);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(FPX_EHIP);
  *out = ctx;
  return FPX_OK;
}

int32_t fpx_destroy(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm) (void)fpx_comm_destroy(ctx);
  free_state(ctx);
  delete ctx;
  return FPX_OK;
}

int32_t fpx_reset(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  return init_state(ctx);
}

int32_t fpx_set_stream(fpx_ctx* ctx, void* hip_stream) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream == FPX_STREAM_OWN ? ctx->own_stream : (hipStream_t)hip_stream;
  return FPX_OK;
}

int32_t fpx_sync(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  return fetch_status(ctx);
}

int32_t fpx_error_detail(fpx_ctx* ctx, int32_t* index, int32_t* slot, int32_t* round) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  if (index) *index = ctx->err_index;
  if (slot) *slot = ctx->err_slot;
  if (round) *round = ctx->err_round;
  return FPX_OK;
}

int32_t fpx_profile_enable(fpx_ctx* ctx, int32_t on) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  if (on && ctx->ev.empty()) {
    ctx->ev.resize(2 * 1024);
    for (auto& e : ctx->ev) HIPCHK(ctx, hipEventCreate(&e));
    ctx->cev.resize(2 * 1024);
    for (auto& e : ctx->cev) HIPCHK(ctx, hipEventCreate(&e));
  }
  ctx->profiling = on != 0;
  ctx->ev_used = 0;
  ctx->cev_used = 0;
  return FPX_OK;
}

int32_t fpx_profile_read(fpx_ctx* ctx, int32_t* launches, double* total_ms) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  double sum = 0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
    sum += ms;
  }
  if (launches) *launches = (int32_t)(ctx->ev_used / 2);
  if (total_ms) *total_ms = sum;
  ctx->ev_used = 0;
  return FPX_OK;
}

int32_t fpx_profile_read_launches(fpx_ctx* ctx, int32_t cap, float* ms_out, int32_t* launches) {
  DeviceGuard _dg(ctx);
  if (!ctx || cap < 0 || (cap > 0 && !ms_out)) return FPX_EINVAL;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int32_t k = 0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2, ++k) {
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
    if (k < cap) ms_out[k] = ms;
  }
  if (launches) *launches = k;
  ctx->ev_used = 0;
  return FPX_OK;
}

int32_t fpx_last_hip_error(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx); return ctx ? ctx->last_hip : 0; }
int32_t fpx_get_config(fpx_ctx* ctx, fpx_config* out) {
  if (!ctx || !out) return FPX_EINVAL;
  *out = ctx->cfg;
  return FPX_OK;
}

int64_t fpx_device_bytes(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx); return ctx ? ctx->bytes : 0; }

int32_t fpx_placement_stats(fpx_ctx* ctx, float out[5]) {
  if (!ctx || !out) return FPX_EINVAL;
  for (int i = 0; i < 5; ++i) out[i] = ctx->placement[i];
  return FPX_OK;
}

int64_t fpx_deferred_folds(fpx_ctx* ctx) { return ctx ? ctx->fins_carried : 0; }

int32_t fpx_placement_search(fpx_ctx* ctx, int32_t* probes, int32_t* unprobed, float* ms) {
  if (!ctx) return FPX_EINVAL;
  if (probes) *probes = ctx->placement_probes;
  if (unprobed) *unprobed = ctx->placement_unprobed;
  if (ms) *ms = ctx->placement_ms;
  return FPX_OK;
}

int32_t fpx_host_alloc(int64_t bytes, void** out) {
  if (!out || bytes <= 0) return FPX_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FPX_ENODEVICE;
  const hipError_t e = hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    return e == hipErrorOutOfMemory ? FPX_ENOMEM : FPX_EHIP;
  }
  return FPX_OK;
}

int32_t fpx_host_free(void* p) {
  if (!p) return FPX_EINVAL;
  return hipHostFree(p) == hipSuccess ? FPX_OK : FPX_EHIP;
}

// ---- a5 --------------------------------------------------------------------------------------------
static int32_t quorum_eval_impl(const fpx_config* cfg, int32_t n, const uint64_t* nodes, int32_t strict, int read,
                                uint8_t* out) {
  if (!cfg || n < 0 || (n > 0 && (!nodes || !out))) return FPX_EINVAL;
  fpx_config c = *cfg;
  // only the quorum fields matter here; make the rest valid
  if (c.num_slots < 1) c.num_slots = 1;
  if (c.num_groups < 1) c.num_groups = 1;
  if (c.num_leader_groups < 1) c.num_leader_groups = 1;
  if (c.num_leaders < 1) c.num_leaders = 1;
  if (c.tally_ways < 1) c.tally_ways = 1;
  int rc = check_config(&c);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FPX_ENODEVICE;
  DeviceGuard _dg(c.device >= 0 && c.device < ndev ? c.device : 0);
  Geom g;
  make_geom(c, &g);
  uint64_t* d_nodes = nullptr;
  uint8_t* d_out = nullptr;
  int32_t* d_status = nullptr;
  fpx_ctx* none = nullptr;
  HIPCHK(none, hipMalloc((void**)&d_nodes, (size_t)n * 32));
  HIPCHK(none, hipMalloc((void**)&d_out, (size_t)n));
  HIPCHK(none, hipMalloc((void**)&d_status, 32));
  HIPCHK(none, hipMemset(d_status, 0, 32));
  HIPCHK(none, hipMemcpy(d_nodes, nodes, (size_t)n * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_quorum_eval, dim3((n + 255) / 256), dim3(256), 0, 0, g, n, d_nodes, strict, read, d_out, d_status);
  HIPCHK(none, hipGetLastError());
  int32_t hs[2] = {0, 0};
  HIPCHK(none, hipMemcpy(out, d_out, (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(none, hipMemcpy(hs, d_status, sizeof(hs), hipMemcpyDeviceToHost));
  (void)hipFree(d_nodes);
  (void)hipFree(d_out);
  (void)hipFree(d_status);
  return hs[0];
}

int32_t fpx_quorum_eval(const fpx_config* cfg, int32_t n, const uint64_t* nodes, int32_t strict, uint8_t* out) {
  return quorum_eval_impl(cfg, n, nodes, strict, 0, out);
}
int32_t fpx_read_quorum_eval(const fpx_config* cfg, int32_t n, const uint64_t* nodes, int32_t strict, uint8_t* out) {
  return quorum_eval_impl(cfg, n, nodes, strict, 1, out);
}
int32_t fpx_is_write_quorum(const fpx_config* cfg, const uint64_t nodes[4], int32_t strict, uint8_t* out) {
  return quorum_eval_impl(cfg, 1, nodes, strict, 0, out);
}

// ---- device-pointer entry points -----------------------------------------------------------------
int32_t fpx_acceptor_phase2a_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                                 const int32_t* d_value_id, const uint64_t* d_target_mask, uint64_t* d_vote_bits,
                                 uint64_t* d_nack_bits, int32_t* d_nack_round) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0) return FPX_EINVAL;
  Batch b = batch_of(n, d_slot, d_round, d_value_id, d_target_mask);
  b.vote_bits = d_vote_bits, b.nack_bits = d_nack_bits, b.nack_round = d_nack_round;
  return enqueue_phase2(ctx, b, false, RunOpts{});
}

int32_t fpx_wire_decode_proxy_leader_inbound_dev(fpx_ctx* ctx, const uint8_t* d_buf, int64_t buf_len,
                                                 const int64_t* d_offsets, int32_t n, int32_t* d_kind, int32_t* d_slot,
                                                 int32_t* d_round, int32_t* d_is_noop, int64_t* d_value_off,
                                                 int32_t* d_value_len, int32_t* d_group_index, int32_t* d_acceptor_index,
                                                 int32_t value_id_base, int32_t* d_value_id) {
  WireOut o{d_kind, d_slot, d_round, d_is_noop, d_value_len, d_group_index, d_acceptor_index, d_value_id, d_value_off,
            value_id_base};
  return wire_decode_dev<0>(ctx, d_buf, buf_len, d_offsets, n, o);
}

int32_t fpx_wire_decode_acceptor_inbound_dev(fpx_ctx* ctx, const uint8_t* d_buf, int64_t buf_len,
                                             const int64_t* d_offsets, int32_t n, int32_t* d_kind, int32_t* d_slot,
                                             int32_t* d_round, int32_t* d_is_noop, int64_t* d_value_off,
                                             int32_t* d_value_len, int32_t* d_chosen_watermark, int32_t value_id_base,
                                             int32_t* d_value_id) {
  WireOut o{d_kind, d_slot, d_round, d_is_noop, d_value_len, d_chosen_watermark, nullptr, d_value_id, d_value_off,
            value_id_base};
  return wire_decode_dev<1>(ctx, d_buf, buf_len, d_offsets, n, o);
}

int32_t fpx_wire_encode_replica_chosen_dev(fpx_ctx* ctx, int32_t n, const uint8_t* d_emit, const int32_t* d_slot,
                                           const int32_t* d_is_noop, const uint8_t* d_values, int64_t values_len,
                                           const int64_t* d_value_off, const int32_t* d_value_len, uint8_t* d_out,
                                           int64_t cap, int64_t* d_out_offsets, int64_t* d_totals) {
  if (!enc_common_ok(ctx, n, d_out, cap, d_out_offsets, n, d_totals) || values_len < 0) return FPX_EINVAL;
  if (n > 0 && (!d_slot || !d_value_off || !d_value_len || (!d_values && values_len > 0))) return FPX_EINVAL;
  DeviceGuard _dg(ctx);
  EncArgs a = {};
  a.n = n, a.emit = d_emit, a.slot = d_slot, a.is_noop = d_is_noop, a.values = d_values, a.values_len = values_len;
  a.value_off = d_value_off, a.value_len = d_value_len;
  a.out = d_out, a.cap = cap, a.max_msgs = n, a.out_offsets = d_out_offsets, a.totals = d_totals;
  return wire_encode_dev<ENC_CHOSEN>(ctx, a);
}

int32_t fpx_wire_encode_phase2b_batch_dev(fpx_ctx* ctx, int32_t dialect, int32_t n, const int32_t* d_slot,
                                          const int32_t* d_round, const uint64_t* d_vote_bits,
                                          const int32_t* d_group_of_slot, int32_t grid_cols, uint8_t* d_out, int64_t cap,
                                          int64_t* d_out_offsets, int64_t max_msgs, int64_t* d_totals) {
  if (!enc_common_ok(ctx, n, d_out, cap, d_out_offsets, max_msgs, d_totals)) return FPX_EINVAL;
  if ((dialect != FPX_WIRE_MULTIPAXOS && dialect != FPX_WIRE_MENCIUS) || (n > 0 && (!d_slot || !d_round || !d_vote_bits)))
    return FPX_EINVAL;
  DeviceGuard _dg(ctx);
  EncArgs a = {};
  a.n = n, a.dialect = dialect, a.grid_cols = grid_cols, a.slot = d_slot, a.round = d_round, a.vote_bits = d_vote_bits;
  a.group_of_slot = d_group_of_slot;
  a.out = d_out, a.cap = cap, a.max_msgs = max_msgs, a.out_offsets = d_out_offsets, a.totals = d_totals;
  return wire_encode_dev<ENC_PHASE2B>(ctx, a);
}

int32_t fpx_wire_encode_leader_nack_dev(fpx_ctx* ctx, int32_t dialect, int32_t n, const int32_t* d_nack_round,
                                        uint8_t* d_out, int64_t cap, int64_t* d_out_offsets, int64_t max_msgs,
                                        int64_t* d_totals) {
  if (!enc_common_ok(ctx, n, d_out, cap, d_out_offsets, max_msgs, d_totals)) return FPX_EINVAL;
  if ((dialect != FPX_WIRE_MULTIPAXOS && dialect != FPX_WIRE_MENCIUS) || (n > 0 && !d_nack_round)) return FPX_EINVAL;
  DeviceGuard _dg(ctx);
  EncArgs a = {};
  a.n = n, a.dialect = dialect, a.round = d_nack_round;
  a.out = d_out, a.cap = cap, a.max_msgs = max_msgs, a.out_offsets = d_out_offsets, a.totals = d_totals;
  return wire_encode_dev<ENC_NACK>(ctx, a);
}

// One proxy-leader tick, bytes to bytes, through the staging driver of the host-pointer entry points (host_runs): the
// tick's bytes and offsets go up, ONE device run decodes, requires Phase2a's, votes and tallies, and encodes the Chosen
// messages, and the reply's bytes, offsets, totals and Nack rounds come down.
int32_t fpx_wire_phase2_tick(fpx_ctx* ctx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets, int32_t n,
                             uint8_t* out, int64_t out_cap, int64_t* out_offsets, int64_t* out_count,
                             int32_t* nack_round, int64_t* bytes_needed, int32_t* bad_index) {
  if (!ctx || n < 0 || n >= (1 << 30) || in_len < 0 || out_cap < 0 || !out_offsets || !out_count) return FPX_EINVAL;
  if (n > 0 && (!in || !in_offsets || (!out && out_cap > 0))) return FPX_EINVAL;
  DeviceGuard _dg(ctx);
  *out_count = 0, out_offsets[0] = 0;
  if (bytes_needed) *bytes_needed = 0;
  if (bad_index) *bad_index = -1;
  if (n == 0) return FPX_OK;
  if (!mapped_host(in) || !mapped_host(in_offsets) || (out && !mapped_host(out)) || !mapped_host(out_offsets) ||
      (nack_round && !mapped_host(nack_round)))
    return FPX_EINVAL;
  int64_t totals[2] = {0, 0};
  uint8_t *d_buf, *d_out, *d_chosen;
  int64_t *d_off, *d_ooff, *d_tot, *value_off;
  int32_t *d_nack, *d_cround, *d_cvalue, *rec[6];  // the decoded records: kind, slot, round, is_noop, value_len, value_id
  const size_t m = (size_t)n;
  const int rc = host_runs(
      ctx, n,
      {fpx::in(d_buf, in, (size_t)in_len), fpx::in(d_off, in_offsets, m + 1), fpx::out(d_out, out, (size_t)out_cap),
       fpx::out(d_ooff, out_offsets, m + 1), fpx::out(d_nack, nack_round, m), fpx::out(d_tot, totals, 2), scratch(rec[0], m),
       scratch(rec[1], m), scratch(rec[2], m), scratch(rec[3], m), scratch(rec[4], m), scratch(rec[5], m), scratch(value_off, m),
       scratch(d_chosen, m), scratch(d_cround, m), scratch(d_cvalue, m)},
      nullptr, [&](int, int, const RunOpts& opts) {
        int r = fpx_wire_decode_proxy_leader_inbound_dev(ctx, d_buf, in_len, d_off, n, rec[0], rec[1], rec[2], rec[3], value_off,
                                                         rec[4], nullptr, nullptr, 0, rec[5]);
        if (r) return r;
        hipLaunchKernelGGL(k_wire_require_kind, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st, rec[0], n,
                           (int32_t)FPX_WIRE_PHASE2A);
        hipLaunchKernelGGL(k_wire_tail, dim3(1), dim3(1), 0, ctx->stream, ctx->st);
        if ((r = launch_check(ctx))) return r;
        r = run_phase2_fused(ctx, n, rec[1], rec[2], rec[5], nullptr, d_chosen, d_cround, d_cvalue, d_nack, opts);
        if (r) return r;
        return fpx_wire_encode_replica_chosen_dev(ctx, n, d_chosen, rec[1], rec[3], d_buf, in_len, value_off, rec[4], d_out,
                                                  out_cap, d_ooff, d_tot);
      });
  if (bad_index && (rc == FPX_EINVAL || rc == FPX_EORDER)) *bad_index = ctx->err_index;
  if (rc != FPX_OK && rc != FPX_ECAPACITY) return rc;
  if (bytes_needed) *bytes_needed = totals[1];
  if (rc == FPX_OK) *out_count = totals[0];
  else out_offsets[0] = 0;
  return rc;
}

int32_t fpx_phase2_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                             const int32_t* d_value_id, const uint64_t* d_target_mask, uint8_t* d_chosen,
                             int32_t* d_chosen_round, int32_t* d_chosen_value, int32_t* d_nack_round) {
  if (!ctx || n < 0) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (by device number: a pending fold of the launch before is this call's to carry)
  return run_phase2_fused(ctx, n, d_slot, d_round, d_value_id, d_target_mask, d_chosen, d_chosen_round, d_chosen_value,
                          d_nack_round, RunOpts{});
}

int32_t fpx_proxy_open_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                           const int32_t* d_value_id, uint8_t* d_is_new) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0) return FPX_EINVAL;
  Batch b = batch_of(n, d_slot, d_round, d_value_id);
  b.is_new = d_is_new;
  return enqueue_open(ctx, b, RunOpts{});
}

int32_t fpx_proxy_phase2b_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                              const uint64_t* d_vote_bits, uint8_t* d_newly_chosen, int32_t* d_chosen_round,
                              int32_t* d_chosen_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0) return FPX_EINVAL;
  Batch b = batch_of(n, d_slot, d_round, nullptr);
  b.vote_bits = const_cast<uint64_t*>(d_vote_bits), b.chosen = d_newly_chosen, b.chosen_round = d_chosen_round, b.chosen_value = d_chosen_value;
  return enqueue_tally(ctx, b, RunOpts{});
}

int32_t fpx_proxy_phase2b_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                   const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_round,
                                   int32_t grid_cols, uint8_t* d_newly_chosen, int32_t* d_chosen_round,
                                   int32_t* d_chosen_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30) || grid_cols < 0) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!d_acceptor_index || !d_slot || !d_round) return FPX_EINVAL;
  MsgBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n, b.kind = d_kind, b.group = d_group_index, b.acceptor = d_acceptor_index, b.slot = d_slot, b.round = d_round;
  b.grid_cols = grid_cols;
  b.chosen = d_newly_chosen, b.chosen_round = d_chosen_round, b.chosen_value = d_chosen_value;
  return enqueue_tally_msgs(ctx, b);
}

// the host form: ONE run through the staging driver (no run contract applies, so there is nothing to cut)
int32_t fpx_proxy_phase2b_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                               const int32_t* acceptor_index, const int32_t* slot, const int32_t* round, int32_t grid_cols,
                               uint8_t* newly_chosen, int32_t* chosen_round, int32_t* chosen_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30) || grid_cols < 0) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!acceptor_index || !slot || !round) return FPX_EINVAL;
  int32_t *d_kind, *d_group, *d_acceptor, *d_slot, *d_round, *d_cround, *d_cvalue;
  uint8_t* d_chosen;
  return host_runs(ctx, n,
                   {opt_in(d_kind, kind, n), opt_in(d_group, group_index, n), in(d_acceptor, acceptor_index, n), in(d_slot, slot, n),
                    in(d_round, round, n), out(d_chosen, newly_chosen, n), out(d_cround, chosen_round, n),
                    out(d_cvalue, chosen_value, n)},
                   nullptr, [&](int, int, const RunOpts&) {
                     return fpx_proxy_phase2b_msgs_dev(ctx, n, d_kind, d_group, d_acceptor, d_slot, d_round, grid_cols, d_chosen,
                                                       d_cround, d_cvalue);
                   });
}

// One tick of a proxy leader among remote acceptors, bytes to records, through the staging driver as ONE run: the tick's
// bytes and offsets go up, the device decodes, tallies the Phase2b's (claim / gather / tally) and compacts the newly
// chosen records in message order; the count and the records come down.
int32_t fpx_wire_phase2b_tick(fpx_ctx* ctx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets, int32_t n,
                              int32_t grid_cols, int32_t* out_slot, int32_t* out_round, int32_t* out_value_id,
                              int32_t out_cap, int32_t* out_count, int32_t* bad_index) {
  if (!ctx || n < 0 || n >= (1 << 30) || in_len < 0 || out_cap < 0 || grid_cols < 0 || !out_count) return FPX_EINVAL;
  if (out_cap > 0 && (!out_slot || !out_round || !out_value_id)) return FPX_EINVAL;
  if (n > 0 && (!in || !in_offsets)) return FPX_EINVAL;
  DeviceGuard _dg(ctx);
  *out_count = 0;
  if (bad_index) *bad_index = -1;
  if (n == 0) return FPX_OK;
  if (!mapped_host(in) || !mapped_host(in_offsets) ||
      (out_cap > 0 && (!mapped_host(out_slot) || !mapped_host(out_round) || !mapped_host(out_value_id))))
    return FPX_EINVAL;
  MsgCompact c;
  memset(&c, 0, sizeof(c));
  c.n = n, c.nblk = (n + 255) / 256, c.cap = out_cap;
  int64_t totals[2] = {0, 0};
  uint8_t *d_buf, *d_chosen;
  int64_t* d_off;
  int32_t *d_cround, *d_cvalue, *r5[5];  // the decoded records: kind, slot, round, group_index, acceptor_index
  const size_t m = (size_t)n, cap = (size_t)out_cap;
  const int rc = host_runs(
      ctx, n,
      {fpx::in(d_buf, in, (size_t)in_len), fpx::in(d_off, in_offsets, m + 1), out(c.out_slot, out_slot, cap),
       out(c.out_round, out_round, cap), out(c.out_value, out_value_id, cap), out(c.totals, totals, 2), scratch(r5[0], m),
       scratch(r5[1], m), scratch(r5[2], m), scratch(r5[3], m), scratch(r5[4], m), scratch(d_chosen, m), scratch(d_cround, m),
       scratch(d_cvalue, m), scratch(c.blk, (size_t)c.nblk)},
      nullptr, [&](int, int, const RunOpts&) {
        int r = fpx_wire_decode_proxy_leader_inbound_dev(ctx, d_buf, in_len, d_off, n, r5[0], r5[1], r5[2], nullptr, nullptr,
                                                         nullptr, r5[3], r5[4], 0, nullptr);
        if (r) return r;
        r = fpx_proxy_phase2b_msgs_dev(ctx, n, r5[0], r5[3], r5[4], r5[1], r5[2], grid_cols, d_chosen, d_cround, d_cvalue);
        if (r) return r;
        c.chosen = d_chosen, c.slot = r5[1], c.chosen_round = d_cround, c.chosen_value = d_cvalue;
        hipLaunchKernelGGL(k_msgs_count, dim3(c.nblk), dim3(256), 0, ctx->stream, ctx->st, c);
        hipLaunchKernelGGL(k_msgs_scan, dim3(1), dim3(1024), 0, ctx->stream, ctx->st, c);
        hipLaunchKernelGGL(k_msgs_emit, dim3(c.nblk), dim3(256), 0, ctx->stream, ctx->st, c);
        return launch_check(ctx);
      });
  if (bad_index && rc == FPX_EINVAL) *bad_index = ctx->err_index;
  if (rc == FPX_OK || rc == FPX_ECAPACITY || rc == FPX_EFATAL_UNKNOWN_SLOTROUND) *out_count = (int32_t)totals[0];
  return rc;
}

// ---- host-pointer entry points: stage, split into runs, run, copy back ----------------------------
int32_t fpx_acceptor_phase2a(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                             const int32_t* value_id, const uint64_t* target_mask, uint64_t* vote_bits,
                             uint64_t* nack_bits, int32_t* nack_round) {
  DeviceGuard _dg(ctx);
  int rc = check_args(ctx, n, slot, round);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  if (!value_id) return FPX_EINVAL;
  Batch w = batch_of(n, nullptr, nullptr, nullptr);
  const size_t m = (size_t)n;
  return host_runs(ctx, n,
                   {in(w.slot, slot, m), in(w.round, round, m), in(w.value, value_id, m), opt_in(w.target, target_mask, m * 4),
                    out(w.vote_bits, vote_bits, m * 4), nack_bits ? out(w.nack_bits, nack_bits, m * 4) : absent(w.nack_bits),
                    out(w.nack_round, nack_round, m)},
                   message_runs(ctx, n, slot, round, true), [&](int lo, int len, const RunOpts& opts) {
                     Batch b = run_of(w, lo, len);
                     return enqueue_phase2(ctx, b, false, opts);
                   });
}

// Host-pointer K3.  Optimistic: the uploads are followed at once by the whole batch as ONE validated
// device run (k_validate checks ranges and the run contract on the GPU), so a well-formed batch -- the
// common case -- costs no CPU pass over the messages.  Only when the device reports a contract violation
// (nothing was applied) does the host cut the batch into runs itself and replay them.
int32_t fpx_phase2_fused(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                         const uint64_t* target_mask, uint8_t* chosen, int32_t* chosen_round, int32_t* chosen_value,
                         int32_t* nack_round) {
  DeviceGuard _dg(ctx);
  int rc = check_args(ctx, n, slot, round);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  if (!value_id) return FPX_EINVAL;
  if (n >= 4096) {  // page-locked arrays: submit + wait
    bool used = false;
    rc = host_fused_staged(ctx, n, slot, round, value_id, target_mask, chosen, chosen_round, chosen_value, nack_round, &used);
    if (used) return rc;
  }
  // the arrays are staged ONCE: both passes launch from, and download, the same layout of the staging buffer
  Batch w = batch_of(n, nullptr, nullptr, nullptr);
  const size_t m = (size_t)n;
  const std::initializer_list<Staged> arrays = {
      in(w.slot, slot, m), in(w.round, round, m), in(w.value, value_id, m), opt_in(w.target, target_mask, m * 4),
      out(w.chosen, chosen, m), out(w.chosen_round, chosen_round, m), out(w.chosen_value, chosen_value, m),
      out(w.nack_round, nack_round, m)};
  const StageLayout l = lay_stage(arrays);
  if ((rc = stage_arrays(ctx, arrays, l))) return rc;
  auto pass = [&](auto cut) -> int {
    int r = launch_runs(ctx, n, cut, [&](int lo, int len, const RunOpts& opts) {  // (the fold of one run rides in the next run's launch)
      Batch b = run_of(w, lo, len);
      return enqueue_phase2(ctx, b, true, opts);
    });
    if (r || (r = fetch_arrays(ctx, arrays, l))) return r;
    return fetch_status(ctx);
  };
  rc = pass(nullptr);
  if (rc == FPX_EINVAL) return check_inputs(ctx, n, slot, round);  // the FIRST offender, for fpx_error_detail
  if (rc != FPX_EORDER) return rc;
  return pass(message_runs(ctx, n, slot, round, true));  // the host-split replay: the inputs are still staged
}

int32_t fpx_phase2_fused_submit(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                                const uint64_t* target_mask, uint8_t* chosen, int32_t* chosen_round, int32_t* chosen_value,
                                int32_t* nack_round, int32_t* ticket) {
  if (!ctx) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (by device number, like fpx_phase2_fused_dev: the fold of the call before rides in this one's)
  int rc = check_args(ctx, n, slot, round);
  if (rc) return rc;
  if (n == 0 || !value_id || !ticket) return FPX_EINVAL;
  int t = -1;
  rc = host_submit(ctx, n, slot, round, value_id, target_mask, chosen, chosen_round, chosen_value, nack_round, &t);
  *ticket = t;
  return rc;
}

int32_t fpx_phase2_fused_wait(fpx_ctx* ctx, int32_t ticket) {
  if (!ctx) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (waits for an event and reads the call's status words: no state is touched)
  return host_wait(ctx, ticket);
}

int32_t fpx_proxy_open(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                       uint8_t* is_new) {
  DeviceGuard _dg(ctx);
  int rc = check_args(ctx, n, slot, round);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  if (!value_id) return FPX_EINVAL;
  Batch w = batch_of(n, nullptr, nullptr, nullptr);
  return host_runs(ctx, n, {in(w.slot, slot, n), in(w.round, round, n), in(w.value, value_id, n), out(w.is_new, is_new, n)},
                   message_runs(ctx, n, slot, round, false), [&](int lo, int len, const RunOpts& opts) {
                     Batch b = run_of(w, lo, len);
                     return enqueue_open(ctx, b, opts);
                   });
}

int32_t fpx_proxy_phase2b(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round, const uint64_t* vote_bits,
                          uint8_t* newly_chosen, int32_t* chosen_round, int32_t* chosen_value) {
  DeviceGuard _dg(ctx);
  int rc = check_args(ctx, n, slot, round);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  if (!vote_bits) return FPX_EINVAL;
  Batch w = batch_of(n, nullptr, nullptr, nullptr);
  const size_t m = (size_t)n;
  return host_runs(ctx, n,
                   {in(w.slot, slot, m), in(w.round, round, m), in(w.vote_bits, vote_bits, m * 4), out(w.chosen, newly_chosen, m),
                    out(w.chosen_round, chosen_round, m), out(w.chosen_value, chosen_value, m)},
                   message_runs(ctx, n, slot, round, false), [&](int lo, int len, const RunOpts& opts) {
                     Batch b = run_of(w, lo, len);
                     return enqueue_tally(ctx, b, opts);
                   });
}

// Phase1a on device-resident arguments, asynchronous: d_target_mask 4 words or NULL, d_outp / d_outn 4 words each = promised
// bits, nack bits (both written in full).  With a ballot per cell: ONE launch (k_p1a_fast) that leaves a pending fold pending
// -- the callers enter by device number, like fpx_phase2_fused_dev; FPX_P1A_SPLIT=1 is the order of rounds 2 - 5 (fold,
// k_p1a_decide, k_p1a_sweep as launches of their own).
static int enqueue_phase1a(fpx_ctx* ctx, int group, int round, int watermark, const uint64_t* d_tgt, uint64_t* d_outp,
                           uint64_t* d_outn) {
  int rc;
  const int wm = watermark < 0 ? 0 : watermark;
  const dim3 gr(1), blk(256);  // R <= 256: one block, which also initialises the reply bits
  if (!ctx->g.per_slot) {
    flush_pending_fin(ctx);    // (nothing is ever pending with a round per acceptor)
    hipLaunchKernelGGL(k_phase1a_scalar, gr, blk, 0, ctx->stream, ctx->g, ctx->st, group, round, d_tgt, d_outp, d_outn);
  } else if (wm > ctx->lz_min_from || getenv("FPX_P1A_SPLIT")) {
    // the watermark passes the start of an older lazy promise, maybe (the host knows every watermark it handed in): the
    // cells in between keep the older promise, which k_p1a_sweep first writes into them
    flush_pending_fin(ctx);
    // O(R) unless the Phase1a is stale for some acceptor or an older lazy promise has to be made explicit below
    // the new watermark: k_p1a_sweep returns at once in the common case; when it does sweep, its last block writes
    // the swept acceptors' promises (those none of whose cells was ahead)
    hipLaunchKernelGGL(k_p1a_decide, gr, blk, 0, ctx->stream, ctx->g, ctx->st, group, round, watermark, d_tgt, d_outp, d_outn);
    hipLaunchKernelGGL(k_p1a_sweep, dim3(ctx->num_cus * 2), dim3(256), 0, ctx->stream, ctx->g, ctx->st, group, round,
                       watermark, d_outp, d_outn);
    ctx->lz_min_from = std::min(ctx->lz_min_from, wm);
    ctx->lazy_active = true;
  } else {
    // (the pending fold stays pending: the decision takes the launch's bound from its shards of part_all)
    hipLaunchKernelGGL(k_p1a_fast, dim3(ctx->num_cus * 2), blk, 0, ctx->stream, ctx->g, ctx->st,
                       ctx->pending_fin.nblk ? ctx->pending_fin.par : -1, group, round, watermark, d_tgt, d_outp, d_outn);
    ctx->lz_min_from = std::min(ctx->lz_min_from, wm);
    ctx->lazy_active = true;
  }
  if ((rc = launch_check(ctx))) return rc;
  return FPX_OK;
}

int32_t fpx_acceptor_phase1a_dev(fpx_ctx* ctx, int32_t group, int32_t round, int32_t chosen_watermark,
                                 const uint64_t* d_target_mask, uint64_t* d_promised_bits, uint64_t* d_nack_bits) {
  if (!ctx || group < 0 || group >= ctx->g.ngroups || round < 0 || round > MAX_ROUND) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (a pending fold stays pending: enqueue_phase1a)
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  uint64_t* d_out = (uint64_t*)ctx->d_scratch.p;  // [8]: promised bits, nack bits the caller does not want
  return enqueue_phase1a(ctx, group, round, chosen_watermark, d_target_mask, d_promised_bits ? d_promised_bits : d_out,
                         d_nack_bits ? d_nack_bits : d_out + 4);
}

int32_t fpx_acceptor_phase1a(fpx_ctx* ctx, int32_t group, int32_t round, int32_t chosen_watermark,
                             const uint64_t* target_mask, uint64_t* promised_bits, uint64_t* nack_bits) {
  if (!ctx || group < 0 || group >= ctx->g.ngroups || round < 0 || round > MAX_ROUND) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  uint64_t* d_out = (uint64_t*)ctx->d_scratch.p;       // [8]: promised bits, nack bits
  uint64_t* d_tgt = target_mask ? d_out + 8 : nullptr;  // [4]
  if (target_mask) HIPCHK(ctx, hipMemcpyAsync(d_tgt, target_mask, 32, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = enqueue_phase1a(ctx, group, round, chosen_watermark, d_tgt, d_out, d_out + 4))) return rc;
  uint64_t h[8];
  HIPCHK(ctx, hipMemcpyAsync(h, d_out, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (promised_bits) memcpy(promised_bits, h, 32);
  if (nack_bits) memcpy(nack_bits, h + 4, 32);
  return FPX_OK;
}

// PER_SLOT: every outstanding lazy promise is written into the cells it covers (one sweep over the ballot array)
// and forgotten; k_phase2 goes back to its lean form.  Readback and digests do this implicitly.
static int flush_promises(fpx_ctx* ctx) {
  if (!ctx->g.per_slot || !ctx->lazy_active) return FPX_OK;
  const Geom& g = ctx->g;
  const dim3 grid(ctx->num_cus * 8);
  if (g.R > 32) hipLaunchKernelGGL(k_lazy_flush<64>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else if (g.R > 16) hipLaunchKernelGGL(k_lazy_flush<32>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else if (g.R > 8) hipLaunchKernelGGL(k_lazy_flush<16>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else if (g.R > 4) hipLaunchKernelGGL(k_lazy_flush<8>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else if (g.R > 2) hipLaunchKernelGGL(k_lazy_flush<4>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else if (g.R > 1) hipLaunchKernelGGL(k_lazy_flush<2>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  else hipLaunchKernelGGL(k_lazy_flush<1>, grid, dim3(256), 0, ctx->stream, g, ctx->st);
  const int nsc = ctx->g.ngroups * ctx->g.R;
  hipLaunchKernelGGL(k_lazy_clear, dim3((nsc + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st);
  int rc = launch_check(ctx);
  if (rc) return rc;
  ctx->lazy_active = false, ctx->lz_min_from = 0x7fffffff;
  return FPX_OK;
}

int32_t fpx_acceptor_flush_promises(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  return flush_promises(ctx);
}

int32_t fpx_proxy_forget(fpx_ctx* ctx, int32_t first_slot, int32_t count) {
  DeviceGuard _dg(ctx);
  if (!ctx || first_slot < 0 || count < 0 || (int64_t)first_slot + count > ctx->g.S) return FPX_EINVAL;
  if (count == 0) return FPX_OK;
  // an empty key word is all a tally entry needs to be free again (values / bitmaps are rewritten on open)
  if (ctx->g.lg_rows) {  // the slots of the range are not neighbours in memory: one thread per slot
    hipLaunchKernelGGL(k_clear_slots, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, first_slot, count, 0);
  } else {
    HIPCHK(ctx, hipMemsetAsync(ctx->st.pl_key + (size_t)first_slot * ctx->g.wp, 0, (size_t)count * ctx->g.wp * 4,
                               ctx->stream));
  }
  if (ctx->rt[0].key) {
    // the noop-range tallies that lie inside the window go too: the survivors move to the other table buffer
    const RangeTable& from = ctx->rt[ctx->rt_cur];
    const RangeTable& to = ctx->rt[ctx->rt_cur ^ 1];
    int rc = clear_range_table(ctx, to);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ranges_rehash, dim3((from.cap + 255) / 256), dim3(256), 0, ctx->stream, from, to,
                       ctx->g.num_groups * 4, first_slot, count);
    ++ctx->range_census[FPX_RANGE_CENSUS_REHASH];
    if ((rc = launch_check(ctx))) return rc;
    ctx->rt_cur ^= 1;
  }
  return FPX_OK;
}

int32_t fpx_recycle_slots(fpx_ctx* ctx, int32_t first_slot, int32_t count) {
  DeviceGuard _dg(ctx);
  if (!ctx || first_slot < 0 || count < 0 || (int64_t)first_slot + count > ctx->g.S) return FPX_EINVAL;
  if (count == 0) return FPX_OK;
  if (ctx->g.lg_rows) {
    hipLaunchKernelGGL(k_clear_slots, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, first_slot, count, 1);
  } else {
    const size_t row = (size_t)ctx->g.VS * 4, at = (size_t)first_slot * row, len = (size_t)count * row;
    HIPCHK(ctx, hipMemsetAsync((char*)ctx->st.vote_round + at, 0xFF, len, ctx->stream));  // -1: no vote
    if (ctx->g.VS == ctx->g.RS) HIPCHK(ctx, hipMemsetAsync((char*)ctx->st.vote_value + at, 0xFF, len, ctx->stream));
    if (ctx->st.row_voted) HIPCHK(ctx, hipMemsetAsync(ctx->st.row_voted + first_slot, 0, (size_t)count, ctx->stream));
  }

  return fpx_proxy_forget(ctx, first_slot, count);
}

// ---- K4: Mencius noop ranges (batched; kernels in fpx_ranges.hpp) -----------------------------------------
static int32_t ranges_ctx_ok(fpx_ctx* ctx, int32_t n) {
  if (!ctx || n < 0) return FPX_EINVAL;
  if (ctx->g.per_slot) return FPX_EINVAL;  // ranges act on the acceptor's `round` scalar (mencius/Acceptor.scala:245-260)
  return FPX_OK;
}

enum { RANGES_FUSED = 0, RANGES_ACCEPTORS = 1, RANGES_OPEN = 2, RANGES_TALLY = 3 };

// one device run of n ranges, launched on `stream`; vote_bits must be present for every mode but RANGES_OPEN
static int enqueue_ranges(fpx_ctx* ctx, RangeBatch& b, int mode, const RunOpts& opts, hipStream_t stream) {
  if (b.n == 0) return FPX_OK;
  const Geom& g = ctx->g;
  const size_t words = (size_t)b.n * g.num_groups * 4;
  b.run_id = ++ctx->run_id;
  b.fused = mode == RANGES_FUSED;
  b.quorum = ctx->cfg.f + 1;
  const int gn = (b.n + 255) / 256;
  const bool acceptors = mode == RANGES_FUSED || mode == RANGES_ACCEPTORS;
  if (opts.validates(ctx)) {
    if (acceptors) fill32(ctx, ctx->st.run_round, -1, (size_t)g.ngroups, stream);
    hipLaunchKernelGGL(k_ranges_validate, dim3(gn), dim3(256), 0, stream, g, ctx->st, b, acceptors ? 1 : 0);
  }
  const RangeTable& rt = ctx->rt[ctx->rt_cur];
  // a few ranges: one workgroup walks clear -> open -> resolve -> acceptors -> tally (fpx_ranges.hpp: k_ranges_chain)
  const long long chain_words = ranges_chain_words(b.n, g.num_groups);
  const bool chain = mode == RANGES_FUSED && b.n <= RANGES_CHAIN_MAX && chain_words <= RANGES_CHAIN_LDS_WORDS &&
                     (long long)b.n * g.num_groups * g.R <= 8 * 1024;
  static const int only[4] = {-1, FPX_RANGE_CENSUS_ACCEPTORS_ONLY, FPX_RANGE_CENSUS_OPEN_ONLY, FPX_RANGE_CENSUS_TALLY_ONLY};
  ++ctx->range_census[mode != RANGES_FUSED ? only[mode] : chain ? FPX_RANGE_CENSUS_CHAIN : FPX_RANGE_CENSUS_STEPS];
  if (chain) {
    allow_lds(k_ranges_chain, (size_t)chain_words * 4 + 64);
    hipLaunchKernelGGL(k_ranges_chain, dim3(1), dim3(1024), (size_t)chain_words * 4, stream, g, ctx->st, rt, b);
  }
  if (acceptors && !chain) {
    fill32(ctx, b.vote_bits, 0, words * 2, stream);
    if (b.nack_bits) fill32(ctx, b.nack_bits, 0, words * 2, stream);
    if (b.nack_round) fill32(ctx, b.nack_round, -1, (size_t)b.n, stream);
  }
  if (!chain && (mode == RANGES_FUSED || mode == RANGES_OPEN)) {
    hipLaunchKernelGGL(k_ranges_open, dim3(gn), dim3(256), 0, stream, g, ctx->st, rt, b, 0);
    hipLaunchKernelGGL(k_ranges_resolve, dim3(gn), dim3(256), 0, stream, g, ctx->st, rt, b);
  }
  if (acceptors) {
    const long long threads = (long long)b.n * g.num_groups * g.R;
    if (!chain)
      hipLaunchKernelGGL(k_ranges_acceptors, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, g, ctx->st, b);
    if (g.lg_rows) {  // leader-group-major rows: a range is one run of rows
      const int gy = std::min(b.n, 4096);
      const int gx = std::max(1, std::min(ctx->num_cus * 16 / gy, 64));
      hipLaunchKernelGGL(k_ranges_fill_lg, dim3(gx, gy), dim3(256), 0, stream, g, ctx->st, b);
      ++ctx->range_census[FPX_RANGE_CENSUS_FILL_LG];
    } else if (b.n <= RF_MAXN && g.num_leader_groups <= RF_MAXL) {
      // (RF_JB rows of L ownership words + the kernel's own 12 static bytes: beyond the default 64 KiB of dynamic LDS
      // the kernel needs the opt-in -- ADVICE r03: L close to 2048 failed every launch with FPX_EHIP)
      allow_lds(k_ranges_fill_rows, (size_t)RF_JB * g.num_leader_groups * 4 + 64);
      // sweep the log rows the ranges touch in memory order (fpx_ranges.hpp)
      hipLaunchKernelGGL(k_ranges_fill_rows, dim3(ctx->num_cus * 8), dim3(256), (size_t)RF_JB * g.num_leader_groups * 4,
                         stream, g, ctx->st, b);
      ++ctx->range_census[FPX_RANGE_CENSUS_FILL_SWEEP];
    } else {
      const int gy = std::min(b.n, 4096);
      const int gx = std::max(1, std::min(ctx->num_cus * 16 / gy, 64));
      hipLaunchKernelGGL(k_ranges_fill, dim3(gx, gy), dim3(256), 0, stream, g, ctx->st, b);
      ++ctx->range_census[FPX_RANGE_CENSUS_FILL_RANGE];
    }
  }
  if (mode == RANGES_TALLY) hipLaunchKernelGGL(k_ranges_open, dim3(gn), dim3(256), 0, stream, g, ctx->st, rt, b, 1);
  if (!chain && (mode == RANGES_FUSED || mode == RANGES_TALLY))
    hipLaunchKernelGGL(k_ranges_tally, dim3(gn), dim3(256), 0, stream, g, ctx->st, rt, b);
  return launch_check(ctx);
}

// the batch of one fused device run of n ranges, its scratch in d_rng (grow may reallocate it: a caller with a side stream
// builds the batch while nothing of that stream is in flight)
static int ranges_fused_batch(fpx_ctx* ctx, int32_t n, const int32_t* d_slot_start, const int32_t* d_slot_end,
                              const int32_t* d_round, const uint64_t* d_target_masks, uint64_t* d_vote_bits, uint64_t* d_nack_bits,
                              int32_t* d_nack_round, uint8_t* d_is_new, uint8_t* d_chosen, RangeBatch* b) {
  memset(b, 0, sizeof(*b));
  int rc = ranges_ctx_ok(ctx, n);
  if (rc || n == 0) return rc;
  const size_t words = (size_t)n * ctx->g.num_groups * 4;
  // scratch: entry[n], and the vote bitmaps when the caller does not want them
  if ((rc = grow(ctx, &ctx->d_rng, (size_t)n * 4 + 64 + (d_vote_bits ? 0 : words * 8)))) return rc;
  b->n = n, b->start = d_slot_start, b->end = d_slot_end, b->round = d_round, b->target = d_target_masks;
  b->entry = (int32_t*)ctx->d_rng.p;
  b->vote_bits = d_vote_bits ? d_vote_bits : (uint64_t*)((char*)ctx->d_rng.p + (((size_t)n * 4 + 63) & ~(size_t)63));
  b->nack_bits = d_nack_bits, b->nack_round = d_nack_round, b->is_new = d_is_new, b->chosen = d_chosen;
  return FPX_OK;
}

int32_t fpx_noop_ranges_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot_start, const int32_t* d_slot_end,
                                  const int32_t* d_round, const uint64_t* d_target_masks, uint64_t* d_vote_bits,
                                  uint64_t* d_nack_bits, int32_t* d_nack_round, uint8_t* d_is_new, uint8_t* d_chosen) {
  DeviceGuard _dg(ctx);
  RangeBatch b;
  const int rc = ranges_fused_batch(ctx, n, d_slot_start, d_slot_end, d_round, d_target_masks, d_vote_bits, d_nack_bits, d_nack_round,
                                    d_is_new, d_chosen, &b);
  return rc ? rc : enqueue_ranges(ctx, b, RANGES_FUSED, RunOpts{}, ctx->stream);
}

// A band whose halves are independent, in TWO launches instead of four (profiles/r05_cfg5.md): the vote kernel with the
// range chain as its first workgroup (k_phase2_band), then the fill with the vote kernel's k_finalize in further rows of
// its grid (k_ranges_fill_lg_fin).  Only for the everyday shape -- groups of at most 32 acceptors on leader-group-major
// rows, dense delivery, a chain that fits the vote kernel's own LDS, more than one workgroup of commands; *done = false
// with nothing enqueued otherwise (the caller takes the serial order).
static int enqueue_band_merged(fpx_ctx* ctx, Batch& b, RangeBatch& rb, const RunOpts& opts, bool* done) {
  *done = false;
  const Geom& g = ctx->g;
  const int G = ctx->lanes_per_slot;
  if (G > 8 || b.target || !g.lg_rows || g.per_slot || getenv("FPX_BAND_SERIAL")) return FPX_OK;
  const long long chain_words = ranges_chain_words(rb.n, g.num_groups);
  if (rb.n > RANGES_CHAIN_MAX || chain_words > RANGES_CHAIN_LDS_WORDS || (long long)rb.n * g.num_groups * g.R > 8 * 1024)
    return FPX_OK;
  b.chunk = chunk_for(ctx, b.n);
  if ((b.n + b.chunk - 1) / b.chunk <= 8) return FPX_OK;  // one workgroup of commands: it finalises itself (`solo`)
  // (the launch's LDS is every workgroup's: the chain may raise it to what still lets six workgroups share a CU)
  const size_t lds = std::max(phase2_lds(ctx, b, true, false, true), (size_t)chain_words * 4);
  if (lds > 26000) return FPX_OK;
  // -- from here on as enqueue_phase2 and enqueue_ranges (FPX_F_TRUSTED: no validation passes) --
  int rc = enqueue_validate(ctx, b, true, opts);
  if (rc) return rc;
  const int grid = grid_for(ctx, b.n);
  if ((b.n + 4 * b.chunk - 1) / (4 * b.chunk) > grid) ++ctx->census[FPX_CENSUS_CAPPED];
  b.solo = 0;
  VoteLaunch vl;
  vl.st = begin_phase2_launch(ctx, b);
  if (++ctx->launch_seq == 0) ctx->launch_seq = 1;
  b.launch_seq = ctx->launch_seq;
  rb.run_id = ++ctx->run_id;
  rb.fused = 1;
  rb.quorum = ctx->cfg.f + 1;
  const bool prof = ctx->profiling && ctx->ev_used + 2 <= ctx->ev.size();
  vl.ev_start = prof ? ctx->ev[ctx->ev_used] : nullptr;
  vl.ev_stop = prof ? ctx->ev[ctx->ev_used + 1] : nullptr;
  launch_band(ctx, vl, b, lds, grid, rb);
  if (prof) ctx->ev_used += 2;
  if ((rc = launch_check(ctx))) return rc;
  const FinJob fj = fin_job_of(ctx, vl.st, b, grid);  // the vote launch's fold: further rows of the fill's grid
  const int gy = std::min(rb.n, 4096);
  const int gx = std::max(1, std::min(ctx->num_cus * 16 / gy, 64));
  const int fin_rows = (fj.nblk + gx - 1) / gx;
  hipLaunchKernelGGL(k_ranges_fill_lg_fin, dim3(gx, gy + fin_rows), dim3(256), 0, ctx->stream, g, vl.st, rb, gy, fin_rows,
                     fj.par, fj.grid, fj.seq, fj.fgx, fj.slices);
  *done = true;
  ++ctx->band_merged_steps;
  ++ctx->range_census[FPX_RANGE_CENSUS_BAND];
  return launch_check(ctx);
}

// One proxy-leader step of Mencius: fpx_phase2_fused_dev on the commands, then fpx_noop_ranges_fused_dev on the ranges --
// and, when the caller says that no leader group has both (`independent`), the two halves in two launches
// (enqueue_band_merged) or side by side: the ranges on the context's second stream between a fork and a join event
// (profiles/r05_cfg5.md).
int32_t fpx_mencius_band_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round, const int32_t* d_value_id,
                                   const uint64_t* d_target_mask, uint8_t* d_chosen, int32_t* d_chosen_round, int32_t* d_chosen_value,
                                   int32_t* d_nack_round, int32_t n_ranges, const int32_t* d_slot_start, const int32_t* d_slot_end,
                                   const int32_t* d_range_round, const uint64_t* d_range_target_masks, uint64_t* d_range_vote_bits,
                                   uint64_t* d_range_nack_bits, int32_t* d_range_nack_round, uint8_t* d_range_is_new,
                                   uint8_t* d_range_chosen, int32_t independent) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n_ranges < 0) return FPX_EINVAL;
  int rc;
  const RunOpts opts{};
  auto commands = [&] {
    return run_phase2_fused(ctx, n, d_slot, d_round, d_value_id, d_target_mask, d_chosen, d_chosen_round, d_chosen_value, d_nack_round, opts);
  };
  RangeBatch rb;
  auto range_batch = [&] {
    return ranges_fused_batch(ctx, n_ranges, d_slot_start, d_slot_end, d_range_round, d_range_target_masks, d_range_vote_bits,
                              d_range_nack_bits, d_range_nack_round, d_range_is_new, d_range_chosen, &rb);
  };
  // the serial order (what the two calls would do: the second one's guard launches the fold the first one left pending)
  auto serial = [&] {
    int r = commands();
    if (r) return r;
    flush_pending_fin(ctx);
    return (r = range_batch()) ? r : enqueue_ranges(ctx, rb, RANGES_FUSED, opts, ctx->stream);
  };
  if (!independent || n == 0 || n_ranges == 0 || ctx->g.per_slot) return serial();
  if (!ctx->band_stream) {
    if (hipStreamCreateWithFlags(&ctx->band_stream, hipStreamNonBlocking) != hipSuccess) return FPX_EHIP;
    if (hipEventCreateWithFlags(&ctx->band_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->band_join, hipEventDisableTiming) != hipSuccess)
      return FPX_EHIP;
  }
  // FPX_DEBUG_CHECKS in the environment: a trusted caller's `independent` is checked all the same (a false claim would let
  // the range chain's plain store of an acceptor's round race with k_finalize's atomicMax: silently wrong state, ADVICE
  // r05).  (Not FPX_DEBUG, which only logs: the check sends the step down the validating path, 0.076 -> 0.087 ms per band.)
  const bool debug_env = getenv("FPX_DEBUG_CHECKS") != nullptr;
  if (opts.validates(ctx) || debug_env) {
    // is the caller's word good?  Checked before anything is applied (FPX_EORDER, nothing applied); the halves themselves
    // then run one after the other: their run-contract checks share one scratch table (State::run_round)
    const int L = ctx->g.num_leader_groups;
    if ((rc = grow(ctx, &ctx->d_band, (size_t)L * 4))) return rc;
    fill32(ctx, (int32_t*)ctx->d_band.p, 0, (size_t)L);
    hipLaunchKernelGGL(k_band_mark, dim3((n_ranges + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, n_ranges, d_slot_start, (int32_t*)ctx->d_band.p);
    hipLaunchKernelGGL(k_band_check, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, n, d_slot, d_round,
                       (const int32_t*)ctx->d_band.p, opts.index_base);
    // a launch that failed here would skip the one check this path exists for, silently
    if ((rc = launch_check(ctx))) return rc;
    return serial();
  }
  // the ranges' scratch is sized here, on the main stream: nothing of the side stream is in flight, the previous step joined
  if ((rc = range_batch())) return rc;
  {
    Batch b = batch_of(n, d_slot, d_round, d_value_id, d_target_mask);
    b.chosen = d_chosen, b.chosen_round = d_chosen_round, b.chosen_value = d_chosen_value, b.nack_round = d_nack_round;
    bool done = false;
    if ((rc = enqueue_band_merged(ctx, b, rb, opts, &done)) || done) return rc;  // (not done: rb is as range_batch left it)
  }
  HIPCHK(ctx, hipEventRecord(ctx->band_fork, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->band_stream, ctx->band_fork, 0));
  rc = enqueue_ranges(ctx, rb, RANGES_FUSED, opts, ctx->band_stream);
  const hipError_t je = hipEventRecord(ctx->band_join, ctx->band_stream);
  const int rc2 = commands();
  if (je == hipSuccess) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->band_join, 0));
  if (je != hipSuccess) return FPX_EHIP;
  return rc ? rc : rc2;
}

int64_t fpx_band_merged_steps(fpx_ctx* ctx) { return ctx ? ctx->band_merged_steps : 0; }

// (no DeviceGuard: reading the census must not launch the pending fold it would then count)
int32_t fpx_vote_launch_census(fpx_ctx* ctx, int32_t cap, int64_t* out, int32_t* n) {
  if (!ctx || cap < 0) return FPX_EINVAL;
  if (out) memcpy(out, ctx->census, sizeof(int64_t) * (size_t)std::min<int32_t>(cap, FPX_CENSUS_WORDS));
  if (n) *n = FPX_CENSUS_WORDS;
  return FPX_OK;
}

int32_t fpx_range_launch_census(fpx_ctx* ctx, int64_t* out, int32_t cap, int32_t* n) {
  if (!ctx || cap < 0) return FPX_EINVAL;
  if (out) memcpy(out, ctx->range_census, sizeof(int64_t) * (size_t)std::min<int32_t>(cap, FPX_RANGE_CENSUS_WORDS));
  if (n) *n = FPX_RANGE_CENSUS_WORDS;
  return FPX_OK;
}

namespace {
struct RangeKey {
  int32_t s, e, r;
  bool operator<(const RangeKey& o) const { return s != o.s ? s < o.s : (e != o.e ? e < o.e : r < o.r); }
};

// host batches: argument check (the first offender for fpx_error_detail) and the cuts that make every piece a run
int check_ranges(fpx_ctx* ctx, int n, const int32_t* start, const int32_t* end, const int32_t* round) {
  for (int i = 0; i < n; ++i)
    if (start[i] < 0 || end[i] < start[i] || end[i] > ctx->g.S || round[i] < 0 || round[i] > MAX_ROUND) {
      ctx->err_index = i, ctx->err_slot = start[i], ctx->err_round = round[i];
      return FPX_EINVAL;
    }
  return FPX_OK;
}

void split_range_runs(fpx_ctx* ctx, int n, const int32_t* start, const int32_t* end, const int32_t* round,
                      bool one_round_per_group, bool distinct_keys, std::vector<int>* cuts) {
  cuts->clear();
  cuts->push_back(0);
  std::vector<int32_t> cur((size_t)ctx->g.num_leader_groups, -1);
  std::vector<int> touched;
  std::set<RangeKey> keys;
  for (int i = 0; i < n; ++i) {
    const int lg = start[i] % ctx->g.num_leader_groups;
    bool cut = one_round_per_group && cur[lg] != -1 && cur[lg] != round[i];
    const RangeKey k{start[i], end[i], round[i]};
    if (distinct_keys && !cut) cut = keys.count(k) != 0;
    if (cut) {
      cuts->push_back(i);
      for (int t : touched) cur[t] = -1;
      touched.clear();
      keys.clear();
    }
    if (cur[lg] == -1) touched.push_back(lg);
    cur[lg] = round[i];
    if (distinct_keys) keys.insert(k);
  }
  cuts->push_back(n);
}
}  // namespace

// host-pointer driver shared by the four host entry points
static int32_t host_ranges(fpx_ctx* ctx, int mode, int32_t n, const int32_t* start, const int32_t* end,
                           const int32_t* round, const uint64_t* target_masks, const uint64_t* votes_in,
                           uint64_t* vote_bits, uint64_t* nack_bits, int32_t* nack_round, uint8_t* is_new,
                           uint8_t* chosen) {
  int rc = ranges_ctx_ok(ctx, n);
  if (rc) return rc;
  if (n == 0) return FPX_OK;
  const bool tally = mode == RANGES_TALLY;
  if (!start || !end || !round || (tally && !votes_in)) return FPX_EINVAL;
  if ((rc = check_ranges(ctx, n, start, end, round))) return rc;
  // per range: int32 start / end / round / entry / nack_round, u8 is_new / chosen, and num_groups x 4 words of target /
  // vote / nack bits; the votes are ONE array that goes up (the tally's input) and comes down
  const size_t per = (size_t)ctx->g.num_groups * 4, m = (size_t)n;
  RangeBatch w;
  memset(&w, 0, sizeof(w));
  return host_runs(
      ctx, n,
      {in(w.start, start, m), in(w.end, end, m), in(w.round, round, m), opt_in(w.target, target_masks, m * per),
       inout(w.vote_bits, votes_in, vote_bits, m * per), out(w.nack_bits, nack_bits, m * per), out(w.nack_round, nack_round, m),
       out(w.is_new, is_new, m), out(w.chosen, chosen, m), scratch(w.entry, m)},
      [&](std::vector<int>* cuts) {
        // one round per leader group in every run: the acceptors' scalar needs it, and the table insert relies on
        // "same (start, end) in one launch => same key"
        split_range_runs(ctx, n, start, end, round, true, tally, cuts);
        return FPX_OK;
      },
      [&](int lo, int len, const RunOpts& opts) {
        RangeBatch b = w;
        b.n = len, b.start += lo, b.end += lo, b.round += lo, b.entry += lo, b.nack_round += lo, b.is_new += lo, b.chosen += lo;
        if (b.target) b.target += lo * per;
        b.vote_bits += lo * per, b.nack_bits += lo * per;
        if (tally) b.votes_in = b.vote_bits;
        return enqueue_ranges(ctx, b, mode, opts, ctx->stream);
      });
}

int32_t fpx_noop_ranges_fused(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                              const int32_t* round, const uint64_t* target_masks, uint64_t* vote_bits,
                              uint64_t* nack_bits, int32_t* nack_round, uint8_t* is_new, uint8_t* chosen) {
  DeviceGuard _dg(ctx);
  return host_ranges(ctx, RANGES_FUSED, n, slot_start, slot_end, round, target_masks, nullptr, vote_bits, nack_bits,
                     nack_round, is_new, chosen);
}

int32_t fpx_acceptor_phase2a_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                                         const int32_t* round, const uint64_t* target_masks, uint64_t* vote_bits,
                                         uint64_t* nack_bits, int32_t* nack_round) {
  DeviceGuard _dg(ctx);
  return host_ranges(ctx, RANGES_ACCEPTORS, n, slot_start, slot_end, round, target_masks, nullptr, vote_bits, nack_bits,
                     nack_round, nullptr, nullptr);
}

int32_t fpx_proxy_open_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                                   const int32_t* round, uint8_t* is_new) {
  DeviceGuard _dg(ctx);
  return host_ranges(ctx, RANGES_OPEN, n, slot_start, slot_end, round, nullptr, nullptr, nullptr, nullptr, nullptr,
                     is_new, nullptr);
}

int32_t fpx_proxy_phase2b_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                                      const int32_t* round, const uint64_t* vote_bits, uint8_t* newly_chosen) {
  DeviceGuard _dg(ctx);
  return host_ranges(ctx, RANGES_TALLY, n, slot_start, slot_end, round, nullptr, vote_bits, nullptr, nullptr, nullptr,
                     nullptr, newly_chosen);
}

// the single-range entry points: batches of one
int32_t fpx_acceptor_phase2a_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round,
                                        const uint64_t* target_masks, uint64_t* vote_bits, uint64_t* nack_bits,
                                        int32_t* nack_round) {
  return fpx_acceptor_phase2a_noop_ranges(ctx, 1, &slot_start, &slot_end, &round, target_masks, vote_bits, nack_bits,
                                          nack_round);
}

int32_t fpx_proxy_open_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, uint8_t* is_new) {
  return fpx_proxy_open_noop_ranges(ctx, 1, &slot_start, &slot_end, &round, is_new);
}

int32_t fpx_proxy_phase2b_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round,
                                     const uint64_t* vote_bits, uint8_t* newly_chosen) {
  return fpx_proxy_phase2b_noop_ranges(ctx, 1, &slot_start, &slot_end, &round, vote_bits, newly_chosen);
}

// ---- mencius.ProxyLeader.handlePhase2b + handlePhase2bNoopRange for per-acceptor messages (fpx_mencius_msgs.hpp) ----
int32_t fpx_mencius_proxy_phase2b_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                           const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_slot_end,
                                           const int32_t* d_round, uint8_t* d_newly_chosen, int32_t* d_chosen_round,
                                           int32_t* d_chosen_value) {
  DeviceGuard _dg(ctx);
  int rc = ranges_ctx_ok(ctx, n);
  if (rc) return rc;
  if (n >= (1 << 30)) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!d_acceptor_index || !d_slot || !d_round) return FPX_EINVAL;
  const RangeTable& rt = ctx->rt[ctx->rt_cur];
  if ((rc = claim_array(ctx, &ctx->mm_claim, (size_t)rt.cap))) return rc;
  MenciusMsgs b;
  memset(&b, 0, sizeof(b));
  b.m.n = n, b.m.kind = d_kind, b.m.acceptor = d_acceptor_index, b.m.slot = d_slot, b.m.round = d_round;
  b.m.chosen = d_newly_chosen, b.m.chosen_round = d_chosen_round, b.m.chosen_value = d_chosen_value;
  if ((rc = prepare_tally_msgs(ctx, b.m))) return rc;
  b.group = d_group_index, b.slot_end = d_slot_end, b.range_kind = FPX_WIRE_PHASE2B_NOOP_RANGE;
  b.claim = (int32_t*)ctx->mm_claim.p, b.quorum = ctx->cfg.f + 1, b.run_id = ++ctx->run_id;
  const dim3 grid((n + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_mm_claim, grid, blk, 0, ctx->stream, ctx->g, ctx->st, rt, b);
  hipLaunchKernelGGL(k_mm_gather, grid, blk, 0, ctx->stream, ctx->g, ctx->st, rt, b);
  hipLaunchKernelGGL(k_mm_tally, grid, blk, 0, ctx->stream, ctx->g, ctx->st, rt, b);
  hipLaunchKernelGGL(k_msgs_tail, dim3(1), dim3(1), 0, ctx->stream, ctx->st, b.m);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver, validated on the device like the _dev form
int32_t fpx_mencius_proxy_phase2b_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                       const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                       const int32_t* round, uint8_t* newly_chosen, int32_t* chosen_round,
                                       int32_t* chosen_value) {
  DeviceGuard _dg(ctx);
  int rc = ranges_ctx_ok(ctx, n);
  if (rc) return rc;
  if (n >= (1 << 30)) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!acceptor_index || !slot || !round) return FPX_EINVAL;
  int32_t *d_kind, *d_group, *d_acceptor, *d_slot, *d_end, *d_round, *d_cround, *d_cvalue;
  uint8_t* d_chosen;
  return host_runs(ctx, n,
                   {opt_in(d_kind, kind, n), opt_in(d_group, group_index, n), in(d_acceptor, acceptor_index, n), in(d_slot, slot, n),
                    opt_in(d_end, slot_end, n), in(d_round, round, n), out(d_chosen, newly_chosen, n),
                    out(d_cround, chosen_round, n), out(d_cvalue, chosen_value, n)},
                   nullptr, [&](int, int, const RunOpts&) {
                     return fpx_mencius_proxy_phase2b_msgs_dev(ctx, n, d_kind, d_group, d_acceptor, d_slot, d_end, d_round, d_chosen,
                                                               d_cround, d_cvalue);
                   });
}

// One tick of a Mencius proxy leader among remote acceptors, decoded arrays to records, through the staging driver as ONE
// run: the arrays go up, the device tallies both kinds (claim / gather / tally) and compacts the newly chosen records in
// message order; the count and the records come down.
int32_t fpx_mencius_phase2b_tick(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                 const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                 const int32_t* round, int32_t* out_kind, int32_t* out_slot, int32_t* out_slot_end,
                                 int32_t* out_round, int32_t* out_value_id, int32_t out_cap, int32_t* out_count) {
  DeviceGuard _dg(ctx);
  int rc = ranges_ctx_ok(ctx, n);
  if (rc) return rc;
  if (n >= (1 << 30) || out_cap < 0 || !out_count) return FPX_EINVAL;
  if (out_cap > 0 && (!out_kind || !out_slot || !out_slot_end || !out_round || !out_value_id)) return FPX_EINVAL;
  *out_count = 0;
  if (n == 0) return FPX_OK;
  if (!acceptor_index || !slot || !round) return FPX_EINVAL;
  MenciusEmit m;
  memset(&m, 0, sizeof(m));
  MsgCompact& c = m.c;
  c.n = n, c.nblk = (n + 255) / 256, c.cap = out_cap;
  int64_t totals[2] = {0, 0};
  int32_t *d_kind, *d_group, *d_acceptor, *d_slot, *d_end, *d_round, *d_cround, *d_cvalue;
  uint8_t* d_chosen;
  const size_t msgs = (size_t)n, cap = (size_t)out_cap;
  rc = host_runs(
      ctx, n,
      {opt_in(d_kind, kind, msgs), opt_in(d_group, group_index, msgs), in(d_acceptor, acceptor_index, msgs), in(d_slot, slot, msgs),
       opt_in(d_end, slot_end, msgs), in(d_round, round, msgs), out(m.out_kind, out_kind, cap), out(c.out_slot, out_slot, cap),
       out(m.out_slot_end, out_slot_end, cap), out(c.out_round, out_round, cap), out(c.out_value, out_value_id, cap),
       out(c.totals, totals, 2), scratch(d_chosen, msgs), scratch(d_cround, msgs), scratch(d_cvalue, msgs),
       scratch(c.blk, (size_t)c.nblk)},
      nullptr, [&](int, int, const RunOpts&) {
        int r = fpx_mencius_proxy_phase2b_msgs_dev(ctx, n, d_kind, d_group, d_acceptor, d_slot, d_end, d_round, d_chosen, d_cround,
                                                   d_cvalue);
        if (r) return r;
        c.chosen = d_chosen, c.slot = d_slot, c.chosen_round = d_cround, c.chosen_value = d_cvalue;
        m.kind = d_kind, m.slot_end = d_end, m.phase2b = FPX_WIRE_PHASE2B, m.range_kind = FPX_WIRE_PHASE2B_NOOP_RANGE;
        hipLaunchKernelGGL(k_msgs_count, dim3(c.nblk), dim3(256), 0, ctx->stream, ctx->st, c);
        hipLaunchKernelGGL(k_msgs_scan, dim3(1), dim3(1024), 0, ctx->stream, ctx->st, c);
        hipLaunchKernelGGL(k_mm_emit, dim3(c.nblk), dim3(256), 0, ctx->stream, ctx->st, m);
        return launch_check(ctx);
      });
  if (rc == FPX_OK || rc == FPX_ECAPACITY || rc == FPX_EFATAL_UNKNOWN_SLOTROUND) *out_count = (int32_t)totals[0];
  return rc;
}

// the proxy leader's tally of one range (parity), as k_ranges_read leaves it: state, num_groups x 4 words of votes,
// capacity, home bucket, bucket
static int32_t read_range_entry(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, std::vector<uint64_t>* h) {
  int rc = ranges_ctx_ok(ctx, 0);
  if (rc) return rc;
  const size_t words = (size_t)ctx->g.num_groups * 4;
  if ((rc = grow(ctx, &ctx->d_scratch, (words + 4) * 8))) return rc;
  hipLaunchKernelGGL(k_ranges_read, dim3(1), dim3(64), 0, ctx->stream, ctx->g, ctx->rt[ctx->rt_cur], slot_start, slot_end,
                     round, (uint64_t*)ctx->d_scratch.p);
  if ((rc = launch_check(ctx))) return rc;
  h->resize(words + 4);
  HIPCHK(ctx, hipMemcpyAsync(h->data(), ctx->d_scratch.p, h->size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

// state 0 = unknown, 1 = Pending, 2 = Done; votes num_groups x 4 words
int32_t fpx_read_range_tally(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, int32_t* state,
                             uint64_t* vote_bits) {
  DeviceGuard _dg(ctx);
  std::vector<uint64_t> h;
  int rc = read_range_entry(ctx, slot_start, slot_end, round, &h);
  if (rc) return rc;
  if (state) *state = (int32_t)h[0];
  if (vote_bits) memcpy(vote_bits, h.data() + 1, (h.size() - 4) * 8);
  return FPX_OK;
}

int32_t fpx_read_range_position(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, int32_t* capacity,
                                int32_t* home_bucket, int32_t* bucket) {
  DeviceGuard _dg(ctx);
  std::vector<uint64_t> h;
  int rc = read_range_entry(ctx, slot_start, slot_end, round, &h);
  if (rc) return rc;
  const size_t at = h.size() - 3;
  if (capacity) *capacity = (int32_t)h[at];
  if (home_bucket) *home_bucket = (int32_t)h[at + 1];
  if (bucket) *bucket = h[at + 2] == ~0ull ? -1 : (int32_t)h[at + 2];
  return FPX_OK;
}

// ---- f1: replica log ------------------------------------------------------------------------------------
int32_t fpx_replica_chosen_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_value_id,
                               const uint8_t* d_mask) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0) return FPX_EINVAL;
  return run_replica_chosen(ctx, n, d_slot, d_value_id, d_mask, RunOpts{});
}

int32_t fpx_replica_state(fpx_ctx* ctx, int32_t* executed_watermark, int32_t* num_chosen) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  int32_t h[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h, ctx->st.log_scalars, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (executed_watermark) *executed_watermark = h[0];
  if (num_chosen) *num_chosen = h[1];
  return FPX_OK;
}

int32_t fpx_replica_chosen(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* value_id, const uint8_t* mask,
                           int32_t* executed_watermark, int32_t* num_chosen) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || (n > 0 && (!slot || !value_id))) return FPX_EINVAL;
  for (int i = 0; i < n; ++i) {
    if ((!mask || mask[i]) && (slot[i] < 0 || slot[i] >= ctx->g.S)) {
      ctx->err_index = i, ctx->err_slot = slot[i], ctx->err_round = -1;
      return FPX_EINVAL;
    }
  }
  // masked-out messages must not trip the slot checks on the device: compact them away
  std::vector<int32_t> s, v;
  s.reserve(n), v.reserve(n);
  for (int i = 0; i < n; ++i)
    if (!mask || mask[i]) s.push_back(slot[i]), v.push_back(value_id[i]);
  const int m = (int)s.size();
  int32_t *d_slot, *d_value;
  const int rc = host_runs(
      ctx, m, {in(d_slot, s.data(), (size_t)m), in(d_value, v.data(), (size_t)m)},
      [&](std::vector<int>* cuts) {
        split_runs(ctx, m, s.data(), nullptr, false, cuts);
        return FPX_OK;
      },
      [&](int lo, int len, const RunOpts& opts) { return run_replica_chosen(ctx, len, d_slot + lo, d_value + lo, nullptr, opts); });
  if (rc == FPX_EHIP || rc == FPX_ENOMEM) return rc;  // (a HIP failure: no scalars to report)
  const int st = fpx_replica_state(ctx, executed_watermark, num_chosen);
  return st ? st : rc;
}

int32_t fpx_replica_chosen_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t* executed_watermark,
                                      int32_t* num_chosen) {
  DeviceGuard _dg(ctx);
  if (!ctx || slot_start < 0 || slot_end > ctx->g.S) return FPX_EINVAL;
  const int stride = ctx->cfg.num_leader_groups;
  const int count = slot_start < slot_end ? (slot_end - slot_start + stride - 1) / stride : 0;
  int32_t first = count;
  if (count > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->st.log_scalars + LG_RANGE_FIRST, &first, 4, hipMemcpyHostToDevice, ctx->stream));
    const int grid = std::max(1, std::min((count + 255) / 256, ctx->num_cus * 8));
    hipLaunchKernelGGL(k_log_range_first, dim3(grid), dim3(256), 0, ctx->stream, ctx->st, slot_start, stride, count);
    hipLaunchKernelGGL(k_log_range_fill, dim3(grid), dim3(256), 0, ctx->stream, ctx->st, slot_start, stride);
    int rc = launch_check(ctx);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&first, ctx->st.log_scalars + LG_RANGE_FIRST, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (first == count) {  // the handler ran to its end: executeLog (mencius/Replica.scala:485)
    hipLaunchKernelGGL(k_log_prep, dim3(1), dim3(256), 0, ctx->stream, ctx->g, ctx->st, 0);
    hipLaunchKernelGGL(k_log_scan, dim3(ctx->num_cus * 4), dim3(256), 0, ctx->stream, ctx->g, ctx->st);
    hipLaunchKernelGGL(k_log_commit, dim3(1), dim3(1), 0, ctx->stream, ctx->st);
    int rc = launch_check(ctx);
    if (rc) return rc;
  }
  int rc = fpx_replica_state(ctx, executed_watermark, num_chosen);
  if (rc) return rc;
  return fetch_status(ctx);
}

// the ReplicaMsgs of a burst over its carved scratch; the claim array is the context's, made by the first call
static int replica_msgs(fpx_ctx* ctx, int32_t n, int nblk, const int32_t* d_kind, const int32_t* d_slot,
                        const int32_t* d_slot_end, const int32_t* d_value_id, const uint8_t* d_mask,
                        const ReplicaMsgsScratch& s, ReplicaMsgs* b) {
  const int rc = claim_array(ctx, &ctx->rm_claim, (size_t)ctx->g.S);
  if (rc) return rc;
  memset(b, 0, sizeof(*b));
  b->n = n, b->nblk = nblk;
  b->nparts = std::max(1, std::min({nblk, ctx->num_cus * 8, LG_MAX_PARTS}));
  b->chosen_kind = FPX_WIRE_CHOSEN, b->range_kind = FPX_WIRE_CHOSEN_NOOP_RANGE;
  b->kind = d_kind, b->slot = d_slot, b->slot_end = d_slot_end, b->value = d_value_id, b->mask = d_mask;
  b->claim = (int32_t*)ctx->rm_claim.p;
  b->hdr = s.hdr, b->parts = s.parts, b->blk = s.blk, b->list = s.list, b->res = s.res;
  return FPX_OK;
}

// mencius.Replica.handleChosen + handleChosenNoopRange for a burst in delivery order (fpx_replica_msgs.hpp): eight launches,
// nothing read by the host in between
int32_t fpx_replica_chosen_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_slot,
                                    const int32_t* d_slot_end, const int32_t* d_value_id, const uint8_t* d_mask) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30)) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  if (!d_kind || !d_slot || !d_slot_end || !d_value_id) return FPX_EINVAL;
  int rc;
  const int nblk = (n + 255) / 256;
  ReplicaMsgsScratch s;  // (rm_buf is not counted in fpx_device_bytes)
  if ((rc = carve(ctx, &ctx->rm_buf, &s, [&](Carver& c) { return lay_replica_msgs(c, nblk, n, LG_MAX_PARTS); })))
    return rc;
  ReplicaMsgs b;
  if ((rc = replica_msgs(ctx, n, nblk, d_kind, d_slot, d_slot_end, d_value_id, d_mask, s, &b))) return rc;
  const dim3 per_msg(b.nblk), blk(256);
  const int sweep = std::min(std::max(b.nblk, ctx->num_cus), ctx->num_cus * 8);
  hipLaunchKernelGGL(k_rm_claim, per_msg, blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_offsets, dim3(1), dim3(1024), 0, ctx->stream, b);
  hipLaunchKernelGGL(k_rm_list, per_msg, blk, 0, ctx->stream, b);
  hipLaunchKernelGGL(k_rm_walk, dim3(ctx->g.num_leader_groups), dim3(RM_WALK_THREADS), 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_apply, dim3(b.nparts), blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_prep, dim3(1), blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_scan, dim3(ctx->num_cus * 4), blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_finish, dim3(sweep), blk, 0, ctx->stream, ctx->g, ctx->st, b);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver, validated on the device like the _dev form
int32_t fpx_replica_chosen_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* slot, const int32_t* slot_end,
                                const int32_t* value_id, const uint8_t* mask, int32_t* executed_watermark,
                                int32_t* num_chosen) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30) || (n > 0 && (!kind || !slot || !slot_end || !value_id))) return FPX_EINVAL;
  int rc = FPX_OK;
  int32_t *d_kind, *d_slot, *d_end, *d_value;
  uint8_t* d_mask;
  if (n > 0)
    rc = host_runs(ctx, n, {in(d_kind, kind, n), in(d_slot, slot, n), in(d_end, slot_end, n), in(d_value, value_id, n), opt_in(d_mask, mask, n)},
                   nullptr, [&](int, int, const RunOpts&) {
                     return fpx_replica_chosen_msgs_dev(ctx, n, d_kind, d_slot, d_end, d_value, d_mask);
                   });
  if (rc == FPX_EHIP || rc == FPX_ENOMEM) return rc;  // (a HIP failure: no scalars to report)
  const int st = fpx_replica_state(ctx, executed_watermark, num_chosen);
  return st ? st : rc;
}

// multipaxos.Replica's inbox for a burst in delivery order: the Chosens as above, and when and with which reply slot
// every read of the burst runs (fpx_replica_inbox.hpp).  Nothing is read by the host between the launches.
int32_t fpx_replica_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_slot,
                              const int32_t* d_value_id, const uint8_t* d_mask, int32_t* d_exec_count,
                              int32_t* d_reply_slot, int32_t* d_order, int32_t* d_counts) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30)) return FPX_EINVAL;
  if (ctx->g.num_leader_groups > 1) return FPX_EINVAL;  // mencius.Replica has no read handlers
  const int nout = (d_exec_count != nullptr) + (d_reply_slot != nullptr) + (d_order != nullptr) + (d_counts != nullptr);
  if (nout != 0 && nout != 4) return FPX_EINVAL;
  if (n == 0 && nout == 0) return FPX_OK;
  if (n > 0 && (!d_kind || !d_slot || !d_value_id)) return FPX_EINVAL;
  int rc;
  const int nblk = std::max(1, (n + 255) / 256);
  const size_t ntiles_max = ((size_t)ctx->g.S + RI_TILE - 1) / RI_TILE;
  ReplicaInboxScratch s;
  if ((rc = carve_counted(ctx, &ctx->ri_buf, &s,
                  [&](Carver& c) { return lay_replica_inbox(c, nblk, ntiles_max, LG_MAX_PARTS, nout != 0); })))
    return rc;
  // the Chosens: fpx_replica_msgs.hpp's kernels on a burst without ranges
  ReplicaMsgs m;
  if ((rc = replica_msgs(ctx, n, nblk, d_kind, d_slot, d_slot, d_value_id, d_mask, s.m, &m))) return rc;
  ReplicaInbox b;
  memset(&b, 0, sizeof(b));
  b.n = n, b.S = ctx->g.S;
  b.kind = d_kind, b.slot = d_slot, b.mask = d_mask;
  b.claim = m.claim, b.mhdr = m.hdr, b.rhdr = s.rhdr, b.hdr = s.hdr, b.blk = m.blk, b.tmax = s.tmax;
  b.key0 = s.sort.key[0], b.val0 = s.sort.val[0];
  b.exec_count = d_exec_count, b.reply_slot = d_reply_slot, b.order = d_order, b.counts = d_counts;
  ReplicaMsgs r = m;  // the reads' counts through k_rm_offsets: its "number of ranges" is the number of reads
  r.hdr = b.rhdr;
  const dim3 per_msg(nblk), blk(256);
  const int sweep = std::min(std::max(nblk, ctx->num_cus), ctx->num_cus * 8);
  hipLaunchKernelGGL(k_ri_claim, per_msg, blk, 0, ctx->stream, ctx->g, ctx->st, b);
  hipLaunchKernelGGL(k_rm_apply, dim3(m.nparts), blk, 0, ctx->stream, ctx->g, ctx->st, m);
  hipLaunchKernelGGL(k_rm_prep, dim3(1), blk, 0, ctx->stream, ctx->g, ctx->st, m);
  hipLaunchKernelGGL(k_rm_scan, dim3(ctx->num_cus * 4), blk, 0, ctx->stream, ctx->g, ctx->st, m);
  if (!nout) {
    hipLaunchKernelGGL(k_rm_finish, dim3(sweep), blk, 0, ctx->stream, ctx->g, ctx->st, m);
    return launch_check(ctx);
  }
  const int tiles_grid = (int)std::max<size_t>(1, std::min<size_t>(ntiles_max, (size_t)ctx->num_cus * 8));
  hipLaunchKernelGGL(k_rm_offsets, dim3(1), dim3(1024), 0, ctx->stream, r);
  hipLaunchKernelGGL(k_ri_tilemax, dim3(tiles_grid), blk, 0, ctx->stream, ctx->st, b);
  hipLaunchKernelGGL(k_ri_tilescan, dim3(1), dim3(RI_SCAN_THREADS), 0, ctx->stream, ctx->st, b);
  hipLaunchKernelGGL(k_ri_execby, dim3(tiles_grid), blk, 0, ctx->stream, b);
  hipLaunchKernelGGL(k_ri_reads, per_msg, blk, 0, ctx->stream, b);
  // keys are 0 .. num_slots + 1: the pass count is fixed per context
  (void)burst_sort(ctx->stream, b.hdr + RI_M, s.sort, (int64_t)ctx->g.S + 1, nblk, d_order);
  hipLaunchKernelGGL(k_ri_finish, dim3(sweep), blk, 0, ctx->stream, ctx->g, ctx->st, b);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver; the outputs come down only when the burst was applied
int32_t fpx_replica_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* slot, const int32_t* value_id,
                          const uint8_t* mask, int32_t* exec_count, int32_t* reply_slot, int32_t* order, int32_t counts[4],
                          int32_t* executed_watermark, int32_t* num_chosen) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0 || n >= (1 << 30) || (n > 0 && (!kind || !slot || !value_id))) return FPX_EINVAL;
  if (ctx->g.num_leader_groups > 1) return FPX_EINVAL;
  if (n > 0 && (!exec_count || !reply_slot || !order)) return FPX_EINVAL;
  if (!counts) return FPX_EINVAL;
  int32_t *d_kind, *d_slot, *d_value, *d_exec, *d_reply, *d_order, *d_counts;
  uint8_t* d_mask;
  const int rc = host_runs(ctx, n,
                           {in(d_kind, kind, n), in(d_slot, slot, n), in(d_value, value_id, n), opt_in(d_mask, mask, n),
                            held(d_exec, exec_count, n), held(d_reply, reply_slot, n), held(d_order, order, n), held(d_counts, counts, 4)},
                           nullptr, [&](int, int, const RunOpts&) {
                             return fpx_replica_inbox_dev(ctx, n, d_kind, d_slot, d_value, d_mask, d_exec, d_reply, d_order, d_counts);
                           });
  if (rc == FPX_EHIP || rc == FPX_ENOMEM) return rc;  // (a HIP failure: no scalars to report)
  const int st = fpx_replica_state(ctx, executed_watermark, num_chosen);  // (synchronises the stream)
  return st ? st : rc;
}

// multipaxos.Acceptor's inbox for a burst of per-acceptor messages in delivery order (fpx_acceptor_inbox.hpp).  Nothing is
// read by the host between the launches.
static int32_t acceptor_inbox_ctx_ok(fpx_ctx* ctx, int32_t n, int32_t grid_cols) {
  if (!ctx || n < 0 || n >= (1 << 30) || grid_cols < 0) return FPX_EINVAL;
  if (ctx->g.per_slot || ctx->g.num_leader_groups != 1) return FPX_EINVAL;  // multipaxos.Acceptor: one round per acceptor
  if (grid_cols > 0 && ctx->g.ngroups != 1) return FPX_EINVAL;             // a grid is ONE acceptor group
  return FPX_OK;
}

// the claim table of the two inbox calls for a burst of n: open-addressed, the next power of two at or above 2 n words,
// grown (and then every word set to its between-calls value) when the burst needs more than the context has
static int32_t ai_claim_table(fpx_ctx* ctx, int32_t n, size_t* tsize_out) {
  int rc;
  size_t tsize = 1024;
  while (tsize < 2 * (size_t)n) tsize <<= 1;
  if (tsize * 8 > ctx->ai_tkey.cap) {  // a new table: every word at its between-calls value
    if ((rc = grow_counted(ctx, &ctx->ai_tkey, tsize * 8))) return rc;
    if ((rc = grow_counted(ctx, &ctx->ai_tval, tsize * 4))) return rc;
    fill32(ctx, ctx->ai_tkey.p, -1, ctx->ai_tkey.cap / 4);
    fill32(ctx, ctx->ai_tval.p, -1, ctx->ai_tval.cap / 4);
  }
  *tsize_out = tsize;
  return FPX_OK;
}

// the part of an AcceptorInbox that both acceptor calls fill alike: the sizes, the carved scratch, the claim table
static int acceptor_inbox_args(fpx_ctx* ctx, int32_t n, const AcceptorInboxScratch& s, AcceptorInbox* b) {
  size_t tsize;
  const int rc = ai_claim_table(ctx, n, &tsize);
  if (rc) return rc;
  b->n = n, b->E = ctx->g.ngroups * ctx->g.R;
  b->hdr = s.hdr, b->tile = s.tile, b->accslot = s.accslot, b->tpos = s.tpos;
  b->fin_round = s.fin_round, b->fin_slot = s.fin_slot;
  b->tkey = (unsigned long long*)ctx->ai_tkey.p, b->tval = (int32_t*)ctx->ai_tval.p, b->tmask = (uint32_t)(tsize - 1);
  return FPX_OK;
}

int32_t fpx_acceptor_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                               const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_round,
                               const int32_t* d_value_id, int32_t grid_cols, int32_t* d_reply_kind, int32_t* d_reply_value) {
  // (the guard launches the fold of a fused step that is still pending: the burst reads promised and max_voted)
  DeviceGuard _dg(ctx);
  int rc;
  if ((rc = acceptor_inbox_ctx_ok(ctx, n, grid_cols))) return rc;
  if (n == 0) return FPX_OK;
  if (!d_kind || !d_acceptor_index || !d_slot || !d_round || !d_value_id) return FPX_EINVAL;
  flush_pending_fin(ctx);
  const Geom& g = ctx->g;
  const int E = g.ngroups * g.R;
  const int nblk = (n + AI_TILE - 1) / AI_TILE;
  AcceptorInboxScratch s;
  if ((rc = carve_counted(ctx, &ctx->ai_buf, &s, [&](Carver& c) { return lay_acceptor_inbox(c, n, E); }))) return rc;
  AcceptorInbox b;
  memset(&b, 0, sizeof(b));
  if ((rc = acceptor_inbox_args(ctx, n, s, &b))) return rc;
  b.grid_cols = grid_cols;
  b.kind = d_kind, b.group = d_group_index, b.acceptor = d_acceptor_index, b.slot = d_slot, b.round = d_round;
  b.value = d_value_id;
  b.reply_kind = d_reply_kind, b.reply_value = d_reply_value;
  const dim3 per_tile(nblk), blk(256);
  const int sweep = std::max(1, std::min(nblk, ctx->num_cus * 8));
  hipLaunchKernelGGL(k_ai_keys, per_tile, blk, 0, ctx->stream, g, ctx->st, b, s.sort.key[0], s.sort.val[0]);
  const int at = burst_sort(ctx->stream, b.hdr + AI_M, s.sort, E, nblk);  // keys are 0 .. E
  b.key = s.sort.key[at], b.perm = s.sort.val[at];
  hipLaunchKernelGGL(k_ai_tilemax<0>, dim3(sweep), blk, 0, ctx->stream, b);
  hipLaunchKernelGGL(k_ai_tilescan, dim3(1), dim3(AI_SCAN_THREADS), 0, ctx->stream, ctx->st, b);
  hipLaunchKernelGGL(k_ai_accept, per_tile, blk, 0, ctx->stream, g, ctx->st, b);
  hipLaunchKernelGGL(k_ai_tilemax<1>, dim3(sweep), blk, 0, ctx->stream, b);
  hipLaunchKernelGGL(k_ai_tilescan, dim3(1), dim3(AI_SCAN_THREADS), 0, ctx->stream, ctx->st, b);
  hipLaunchKernelGGL(k_ai_reads, per_tile, blk, 0, ctx->stream, g, ctx->st, b);
  hipLaunchKernelGGL(k_ai_finish, per_tile, blk, 0, ctx->stream, ctx->st, b);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver (no run contract applies, so there is nothing to cut); the replies
// come down only when the burst was applied
int32_t fpx_acceptor_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                           const int32_t* acceptor_index, const int32_t* slot, const int32_t* round, const int32_t* value_id,
                           int32_t grid_cols, int32_t* reply_kind, int32_t* reply_value) {
  DeviceGuard _dg(ctx);
  int rc;
  if ((rc = acceptor_inbox_ctx_ok(ctx, n, grid_cols))) return rc;
  if (n == 0) return FPX_OK;
  if (!kind || !acceptor_index || !slot || !round || !value_id) return FPX_EINVAL;
  int32_t *d_kind, *d_group, *d_acceptor, *d_slot, *d_round, *d_value, *d_rkind, *d_rvalue;
  return host_runs(ctx, n,
                   {in(d_kind, kind, n), opt_in(d_group, group_index, n), in(d_acceptor, acceptor_index, n), in(d_slot, slot, n),
                    in(d_round, round, n), in(d_value, value_id, n), reply_kind ? held(d_rkind, reply_kind, n) : absent(d_rkind),
                    reply_value ? held(d_rvalue, reply_value, n) : absent(d_rvalue)},
                   nullptr, [&](int, int, const RunOpts&) {
                     return fpx_acceptor_inbox_dev(ctx, n, d_kind, d_group, d_acceptor, d_slot, d_round, d_value, grid_cols, d_rkind,
                                                   d_rvalue);
                   });
}

// mencius.Acceptor's inbox for a burst of per-acceptor messages in delivery order, Phase2aNoopRanges among them
// (fpx_mencius_acceptor_inbox.hpp).  Nothing is read by the host between the launches.
static int32_t mencius_acceptor_inbox_ctx_ok(fpx_ctx* ctx, int32_t n) {
  if (!ctx || n < 0 || n >= (1 << 30)) return FPX_EINVAL;
  if (ctx->g.per_slot || ctx->g.qkind == FPX_Q_GRID) return FPX_EINVAL;  // mencius.Acceptor: one round per acceptor, no grids
  return FPX_OK;
}

int32_t fpx_mencius_acceptor_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                       const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_slot_end,
                                       const int32_t* d_round, const int32_t* d_value_id, int32_t* d_reply_kind,
                                       int32_t* d_reply_value) {
  // (the guard launches the fold of a fused step that is still pending: the burst reads promised and max_voted)
  DeviceGuard _dg(ctx);
  int rc;
  if ((rc = mencius_acceptor_inbox_ctx_ok(ctx, n))) return rc;
  if (n == 0) return FPX_OK;
  if (!d_kind || !d_acceptor_index || !d_slot || !d_slot_end || !d_round || !d_value_id) return FPX_EINVAL;
  flush_pending_fin(ctx);
  const Geom& g = ctx->g;
  const int E = g.ngroups * g.R;
  const int nblk = (n + AI_TILE - 1) / AI_TILE;
  MenciusAcceptorInboxScratch s;
  if ((rc = carve_counted(ctx, &ctx->mai_buf, &s, [&](Carver& c) { return lay_mencius_acceptor_inbox(c, n, E); })))
    return rc;
  MenciusAcceptorInbox b;
  memset(&b, 0, sizeof(b));
  if ((rc = acceptor_inbox_args(ctx, n, s.a, &b.a))) return rc;
  b.a.kind = d_kind, b.a.group = d_group_index, b.a.acceptor = d_acceptor_index, b.a.slot = d_slot, b.a.round = d_round;
  b.a.value = d_value_id, b.slot_end = d_slot_end;
  b.rflag = s.rflag, b.rcnt = s.rcnt;
  b.lent = s.list[0], b.lq0 = s.list[1], b.lq1 = s.list[2], b.lround = s.list[3], b.lidx = s.list[4];
  b.a.reply_kind = d_reply_kind, b.a.reply_value = d_reply_value;
  const dim3 per_tile(nblk), blk(256);
  const int sweep = std::max(1, std::min(nblk, ctx->num_cus * 8));
  hipLaunchKernelGGL(k_mai_keys, per_tile, blk, 0, ctx->stream, g, ctx->st, b, s.a.sort.key[0], s.a.sort.val[0]);
  const int at = burst_sort(ctx->stream, b.a.hdr + AI_M, s.a.sort, E, nblk);  // keys are 0 .. E
  b.a.key = s.a.sort.key[at], b.a.perm = s.a.sort.val[at];
  hipLaunchKernelGGL(k_ai_tilemax<2>, dim3(sweep), blk, 0, ctx->stream, b.a);
  hipLaunchKernelGGL(k_ai_tilescan, dim3(1), dim3(AI_SCAN_THREADS), 0, ctx->stream, ctx->st, b.a);
  hipLaunchKernelGGL(k_mai_accept, per_tile, blk, 0, ctx->stream, g, ctx->st, b);
  hipLaunchKernelGGL(k_mai_offsets, dim3(1), dim3(AI_SCAN_THREADS), 0, ctx->stream, b);
  hipLaunchKernelGGL(k_mai_list, per_tile, blk, 0, ctx->stream, g, b);
  hipLaunchKernelGGL(k_ai_tilemax<1>, dim3(sweep), blk, 0, ctx->stream, b.a);
  hipLaunchKernelGGL(k_ai_tilescan, dim3(1), dim3(AI_SCAN_THREADS), 0, ctx->stream, ctx->st, b.a);
  hipLaunchKernelGGL(k_mai_points, per_tile, blk, 0, ctx->stream, g, ctx->st, b);
  // (the list's length stays on the device: the grid is sized by what the burst could hold)
  hipLaunchKernelGGL(k_mai_ranges, dim3(4, std::max(1, std::min(n, ctx->num_cus * 4))), blk, 0, ctx->stream, g, ctx->st, b);
  hipLaunchKernelGGL(k_ai_finish, per_tile, blk, 0, ctx->stream, ctx->st, b.a);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver; the replies come down only when the burst was applied
int32_t fpx_mencius_acceptor_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                   const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                   const int32_t* round, const int32_t* value_id, int32_t* reply_kind,
                                   int32_t* reply_value) {
  DeviceGuard _dg(ctx);
  int rc;
  if ((rc = mencius_acceptor_inbox_ctx_ok(ctx, n))) return rc;
  if (n == 0) return FPX_OK;
  if (!kind || !acceptor_index || !slot || !slot_end || !round || !value_id) return FPX_EINVAL;
  int32_t *d_kind, *d_group, *d_acceptor, *d_slot, *d_end, *d_round, *d_value, *d_rkind, *d_rvalue;
  return host_runs(ctx, n,
                   {in(d_kind, kind, n), opt_in(d_group, group_index, n), in(d_acceptor, acceptor_index, n), in(d_slot, slot, n),
                    in(d_end, slot_end, n), in(d_round, round, n), in(d_value, value_id, n),
                    reply_kind ? held(d_rkind, reply_kind, n) : absent(d_rkind),
                    reply_value ? held(d_rvalue, reply_value, n) : absent(d_rvalue)},
                   nullptr, [&](int, int, const RunOpts&) {
                     return fpx_mencius_acceptor_inbox_dev(ctx, n, d_kind, d_group, d_acceptor, d_slot, d_end, d_round, d_value,
                                                           d_rkind, d_rvalue);
                   });
}

int32_t fpx_replica_read_log(fpx_ctx* ctx, int32_t first, int32_t count, int32_t* values, uint8_t* present) {
  DeviceGuard _dg(ctx);
  if (!ctx || first < 0 || count < 0 || (int64_t)first + count > ctx->g.S) return FPX_EINVAL;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (values && count) HIPCHK(ctx, hipMemcpy(values, ctx->st.log_value + first, (size_t)count * 4, hipMemcpyDeviceToHost));
  if (present && count) HIPCHK(ctx, hipMemcpy(present, ctx->st.log_present + first, (size_t)count, hipMemcpyDeviceToHost));
  return FPX_OK;
}

// ---- f2: Phase-1 recovery scan ------------------------------------------------------------------------
int32_t fpx_leader_phase1b_scan(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* quorum_masks, int32_t cap,
                                int32_t* max_slot, int32_t* safe_round, int32_t* safe_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || !quorum_masks || chosen_watermark < 0 || cap < 0) return FPX_EINVAL;
  const int ng = ctx->g.ngroups;
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, (size_t)ng * 32 + 64 + (size_t)cap * 8))) return rc;
  uint64_t* d_q = (uint64_t*)ctx->d_scratch.p;
  int32_t *d_max = (int32_t*)(d_q + (size_t)ng * 4), *d_sr = d_max + 16, *d_sv = d_sr + cap;
  HIPCHK(ctx, hipMemcpyAsync(d_q, quorum_masks, (size_t)ng * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_max, 0xFF, 4, ctx->stream));
  const int ntab = ng * ctx->g.R;
  hipLaunchKernelGGL(k_quorum_max_slot, dim3((ntab + 255) / 256), dim3(256), 0, ctx->stream, ctx->g, ctx->st, d_q,
                     chosen_watermark, d_max);
  if ((rc = launch_check(ctx))) return rc;
  int32_t hmax = -1;
  HIPCHK(ctx, hipMemcpyAsync(&hmax, d_max, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (max_slot) *max_slot = hmax;
  // for (slot <- chosenWatermark to maxSlot)   Leader.scala:553
  const int64_t want = (int64_t)hmax - chosen_watermark + 1;
  const int count = (int)std::max<int64_t>(0, std::min<int64_t>(want, cap));
  if (count == 0) return FPX_OK;
  switch (ctx->lanes_per_slot) {
    case 1: launch_p1b<1>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    case 2: launch_p1b<2>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    case 4: launch_p1b<4>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    case 8: launch_p1b<8>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    case 16: launch_p1b<16>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    case 32: launch_p1b<32>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
    default: launch_p1b<64>(ctx, d_q, chosen_watermark, count, d_sr, d_sv); break;
  }
  if ((rc = launch_check(ctx))) return rc;
  if (safe_round) HIPCHK(ctx, hipMemcpyAsync(safe_round, d_sr, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (safe_value) HIPCHK(ctx, hipMemcpyAsync(safe_value, d_sv, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

// ---- Leader.handlePhase1b for a burst of Phase1b messages (fpx_phase1b_msgs.hpp) -----------------------------------
int32_t fpx_leader_phase1b_msgs_dev(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, int32_t leader_group,
                                    int32_t recover_slot, uint32_t flags, int32_t n, const int32_t* d_kind,
                                    const int32_t* d_msg_round, const int32_t* d_group_index, const int32_t* d_acceptor_index,
                                    const int64_t* d_offsets, const int32_t* d_info_slot, const int32_t* d_info_vote_round,
                                    const int32_t* d_info_value_id, int32_t grid_cols, int32_t cap, int32_t* d_out_slot,
                                    int32_t* d_safe_round, int32_t* d_safe_value, int64_t* d_result, uint64_t* d_held_bits) {
  if (!ctx || !d_result ||
      !p1m_scalars_ok(ctx->g.num_groups, ctx->g.num_leader_groups, round, MAX_ROUND, chosen_watermark, leader_group,
                      recover_slot, flags, FPX_P1B_GRID_ALL_ROWS, n, grid_cols, cap) ||
      (n > 0 && (!d_msg_round || !d_acceptor_index || !d_offsets)) || (cap > 0 && (!d_out_slot || !d_safe_round || !d_safe_value)))
    return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (no acceptor, tally or replica state is read: a pending fold stays pending)
  const Geom& g = ctx->g;
  const P1mLayout l = p1m_layout(n, g.num_groups, g.ngroups, grid_cols);
  int rc;
  if ((rc = grow(ctx, &ctx->p1m_buf, l.bytes))) return rc;
  if ((rc = grow(ctx, &ctx->p1m_tab, (size_t)cap * 8))) return rc;
  char* base = (char*)ctx->p1m_buf.p;
  P1mArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n, a.round = round, a.leader_group = leader_group, a.recover_slot = recover_slot, a.watermark = chosen_watermark;
  a.all_rows = (flags & FPX_P1B_GRID_ALL_ROWS) ? 1 : 0, a.grid_cols = grid_cols, a.need = ctx->cfg.f + 1;
  a.phase1b = FPX_WIRE_PHASE1B, a.cap = cap;
  a.kind = d_kind, a.msg_round = d_msg_round, a.group = d_group_index, a.acceptor = d_acceptor_index, a.offsets = d_offsets;
  a.info_slot = d_info_slot, a.info_round = d_info_vote_round, a.info_value = d_info_value_id;
  a.keys = l.keys;
  a.ctl = (unsigned long long*)(base + l.ctl), a.held = (unsigned long long*)(base + l.held);
  a.unit0 = (int64_t*)(base + l.unit0), a.first = (int32_t*)(base + l.first), a.last = (int32_t*)(base + l.last);
  a.win = (int32_t*)(base + l.win), a.table = (unsigned long long*)ctx->p1m_tab.p;
  a.out_slot = d_out_slot, a.safe_round = d_safe_round, a.safe_value = d_safe_value, a.result = d_result, a.held_out = d_held_bits;
  HIPCHK(ctx, hipMemsetAsync(base, 0, l.zero_bytes, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(a.first, 0x7f, (size_t)l.keys * 4, ctx->stream));  // 0x7f7f7f7f: above any message index
  HIPCHK(ctx, hipMemsetAsync(a.last, 0xFF, (size_t)l.keys * 4, ctx->stream));
  const dim3 blk(256), sweep(ctx->num_cus * 8);
  if (n > 0) hipLaunchKernelGGL(k_p1m_headers, dim3((n + 255) / 256), blk, 0, ctx->stream, g, ctx->st, a);
  hipLaunchKernelGGL(k_p1m_decide, dim3(1), dim3(1024), 0, ctx->stream, g, ctx->st, a);
  hipLaunchKernelGGL(k_p1m_plan, dim3(1), dim3(1024), 0, ctx->stream, g, a);
  hipLaunchKernelGGL(k_p1m_clear, sweep, blk, 0, ctx->stream, a);
  hipLaunchKernelGGL(k_p1m_walk<false>, sweep, blk, 0, ctx->stream, g, a);
  hipLaunchKernelGGL(k_p1m_walk<true>, sweep, blk, 0, ctx->stream, g, a);
  hipLaunchKernelGGL(k_p1m_fill, sweep, blk, 0, ctx->stream, g, ctx->st, a);
  return launch_check(ctx);
}

// the host form: ONE run through the staging driver; the offsets are checked here first, because they size the uploads
int32_t fpx_leader_phase1b_msgs(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, int32_t leader_group,
                                int32_t recover_slot, uint32_t flags, int32_t n, const int32_t* kind, const int32_t* msg_round,
                                const int32_t* group_index, const int32_t* acceptor_index, const int64_t* offsets,
                                const int32_t* info_slot, const int32_t* info_vote_round, const int32_t* info_value_id,
                                int32_t grid_cols, int32_t cap, int32_t* out_slot, int32_t* safe_round, int32_t* safe_value,
                                int64_t* result, uint64_t* held_bits) {
  if (!ctx || !result ||
      !p1m_scalars_ok(ctx->g.num_groups, ctx->g.num_leader_groups, round, MAX_ROUND, chosen_watermark, leader_group,
                      recover_slot, flags, FPX_P1B_GRID_ALL_ROWS, n, grid_cols, cap) ||
      (n > 0 && (!msg_round || !acceptor_index || !offsets)) || (cap > 0 && (!out_slot || !safe_round || !safe_value)))
    return FPX_EINVAL;
  int32_t bad = -1;
  const int64_t total = p1m_check_offsets(n, offsets, &bad);
  if (total < 0) {
    ctx->err_index = bad, ctx->err_slot = -1, ctx->err_round = msg_round[bad];
    return FPX_EINVAL;
  }
  if (total > 0 && (!info_slot || !info_vote_round || !info_value_id)) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);
  const size_t m = (size_t)n, rec = (size_t)total, outs = (size_t)cap, heldw = (size_t)ctx->g.ngroups * 4;
  const int64_t zero = 0;
  int64_t res[8];
  int32_t *d_kind, *d_msg_round, *d_group, *d_acceptor, *d_is, *d_ir, *d_iv, *d_out_slot, *d_sr, *d_sv;
  int64_t *d_off, *d_res;
  uint64_t* d_held;
  // (n == 0: one zero offset goes up; -1 in every result word: "not written" -- a refused call writes none, an incomplete
  // one two)
  const int rc = host_runs(
      ctx, n,
      {opt_in(d_kind, kind, m), in(d_msg_round, msg_round, m), opt_in(d_group, group_index, m), in(d_acceptor, acceptor_index, m),
       in(d_off, n > 0 ? offsets : &zero, m + 1), in(d_is, info_slot, rec), in(d_ir, info_vote_round, rec),
       in(d_iv, info_value_id, rec), scratch(d_out_slot, outs), scratch(d_sr, outs), scratch(d_sv, outs), out(d_res, res, 8, 0xFF),
       scratch(d_held, heldw)},
      nullptr, [&](int, int, const RunOpts&) {
        return fpx_leader_phase1b_msgs_dev(ctx, round, chosen_watermark, leader_group, recover_slot, flags, n, d_kind, d_msg_round,
                                           d_group, d_acceptor, d_off, d_is, d_ir, d_iv, grid_cols, cap, d_out_slot, d_sr, d_sv,
                                           d_res, d_held);
      });
  if (rc == FPX_EHIP || rc == FPX_ENOMEM || rc == FPX_EINVAL) return rc;
  // what the device wrote, and no more, reaches the caller's arrays
  if (res[0] == 0) {
    result[0] = 0;
    if (res[1] == -1) result[1] = -1;
  } else if (res[0] == 1) {
    for (int w = 0; w < 6; ++w) result[w] = res[w];
    // the first res[5] records and the held bits, from the staging buffer, which keeps them until the next call
    const size_t wr = (size_t)res[5] * 4;
    const std::pair<void*, const void*> down[3] = {{out_slot, d_out_slot}, {safe_round, d_sr}, {safe_value, d_sv}};
    for (const auto& a : down)
      if (a.first && wr) HIPCHK(ctx, hipMemcpyAsync(a.first, a.second, wr, hipMemcpyDeviceToHost, ctx->stream));
    if (held_bits) HIPCHK(ctx, hipMemcpyAsync(held_bits, d_held, heldw * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return rc;
}

// ---- readback ----------------------------------------------------------------------------------------
int32_t fpx_read_state(fpx_ctx* ctx, int32_t* vote_round, int32_t* vote_value, int32_t* ballot) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  const size_t S = (size_t)ctx->g.S, R = (size_t)ctx->g.R, RS = (size_t)ctx->g.RS;
  if (ballot) {
    int rcf = flush_promises(ctx);
    if (rcf) return rcf;
  }
  if (ctx->st.vote_sum && (vote_round || vote_value)) {  // whole arrays are copied: compact rows become cells first
    hipLaunchKernelGGL(k_expand_rows, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, ctx->g, ctx->st);
    int rce = launch_check(ctx);
    if (rce) return rce;
    ctx->may_compact = false;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  // device rows are RS cells long, the caller's are R
  // leader-group-major rows: leader group lg's rows are contiguous on the device and every L-th row of the caller's array
  const size_t L = ctx->g.lg_rows ? (size_t)ctx->g.num_leader_groups : 1, rows = S / L;
  auto fetch = [&](int32_t* dst, const int32_t* src, size_t src_stride) -> int {
    for (size_t lg = 0; lg < L; ++lg)
      HIPCHK(ctx, hipMemcpy2D(dst + lg * R, L * R * 4, src + lg * rows * src_stride, src_stride * 4, R * 4, rows, hipMemcpyDeviceToHost));
    return FPX_OK;
  };
  int rc2;
  if (vote_round && (rc2 = fetch(vote_round, ctx->st.vote_round, (size_t)ctx->g.VS))) return rc2;
  if (vote_value && (rc2 = fetch(vote_value, ctx->st.vote_value, (size_t)ctx->g.VS))) return rc2;
  if (ballot) {
    if (ctx->st.ballot) {
      if ((rc2 = fetch(ballot, ctx->st.ballot, RS))) return rc2;
    } else {
      std::fill(ballot, ballot + S * R, -1);
    }
  }
  return FPX_OK;
}

int32_t fpx_read_scalars(fpx_ctx* ctx, int32_t* promised, int32_t* max_voted_slot) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  const size_t nsc = (size_t)ctx->g.ngroups * ctx->g.R;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (promised) HIPCHK(ctx, hipMemcpy(promised, ctx->st.promised, nsc * 4, hipMemcpyDeviceToHost));
  if (max_voted_slot) HIPCHK(ctx, hipMemcpy(max_voted_slot, ctx->st.max_voted, nsc * 4, hipMemcpyDeviceToHost));
  return FPX_OK;
}

int32_t fpx_read_acceptor(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t* promised, int32_t* max_voted_slot,
                          int32_t* vote_round, int32_t* vote_value, int32_t* ballot) {
  DeviceGuard _dg(ctx);
  if (!ctx || group < 0 || group >= ctx->g.ngroups || replica < 0 || replica >= ctx->g.R) return FPX_EINVAL;
  const size_t e = (size_t)group * ctx->g.R + replica;
  const size_t S = (size_t)ctx->g.S;
  int rc;
  if (ballot && (rc = flush_promises(ctx))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (promised) {
    if (ctx->g.per_slot) *promised = -1;
    else HIPCHK(ctx, hipMemcpy(promised, ctx->st.promised + e, 4, hipMemcpyDeviceToHost));
  }
  if (max_voted_slot) HIPCHK(ctx, hipMemcpy(max_voted_slot, ctx->st.max_voted + e, 4, hipMemcpyDeviceToHost));
  if (vote_round || vote_value || ballot) {
    if ((rc = grow(ctx, &ctx->d_scratch, S * 12 + 128))) return rc;
    int32_t* base = (int32_t*)((char*)ctx->d_scratch.p + 128);
    hipLaunchKernelGGL(k_gather_acceptor, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, ctx->g, ctx->st,
                       group, replica, base, base + S, base + 2 * S);
    if ((rc = launch_check(ctx))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (vote_round) HIPCHK(ctx, hipMemcpy(vote_round, base, S * 4, hipMemcpyDeviceToHost));
    if (vote_value) HIPCHK(ctx, hipMemcpy(vote_value, base + S, S * 4, hipMemcpyDeviceToHost));
    if (ballot) HIPCHK(ctx, hipMemcpy(ballot, base + 2 * S, S * 4, hipMemcpyDeviceToHost));
  }
  return FPX_OK;
}

int32_t fpx_acceptor_max_voted_in(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t first_slot, int32_t count,
                                  int32_t* max_slot) {
  DeviceGuard _dg(ctx);
  if (!ctx || !max_slot || group < 0 || group >= ctx->g.ngroups || replica < 0 || replica >= ctx->g.R || first_slot < 0 || count < 0 ||
      (int64_t)first_slot + count > ctx->g.S)
    return FPX_EINVAL;
  *max_slot = -1;
  if (count == 0) return FPX_OK;
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  int32_t* d = (int32_t*)ctx->d_scratch.p;
  fill32(ctx, d, -1, 1);
  hipLaunchKernelGGL(k_max_voted_in, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, ctx->g, ctx->st, group, replica,
                     first_slot, count, d);
  if ((rc = launch_check(ctx))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(max_slot, d, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

// Acceptor.handlePhase1a's Phase1b.info (multipaxos/Acceptor.scala:166-178): the acceptor's votes in slots >=
// chosen_watermark, ascending (states.iteratorFrom).  Phase 1 is off the steady path: one gather of the acceptor's
// column, compacted on the host.
int32_t fpx_acceptor_phase1b_info(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t chosen_watermark, int32_t cap,
                                  int32_t* count, int32_t* slot, int32_t* vote_round, int32_t* vote_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || !count || cap < 0 || group < 0 || group >= ctx->g.ngroups || replica < 0 || replica >= ctx->g.R ||
      (cap > 0 && (!slot || !vote_round || !vote_value)))
    return FPX_EINVAL;
  *count = 0;
  const size_t e = (size_t)group * ctx->g.R + replica;
  const int64_t S = ctx->g.S;
  int rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int32_t max_voted = -1;
  HIPCHK(ctx, hipMemcpy(&max_voted, ctx->st.max_voted + e, 4, hipMemcpyDeviceToHost));
  const int64_t lo = chosen_watermark < 0 ? 0 : chosen_watermark;
  if (max_voted < lo || lo >= S) return FPX_OK;  // no vote at or above the watermark
  if ((rc = grow(ctx, &ctx->d_scratch, (size_t)S * 12 + 128))) return rc;
  int32_t* base = (int32_t*)((char*)ctx->d_scratch.p + 128);
  hipLaunchKernelGGL(k_gather_acceptor, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, ctx->g, ctx->st,
                     group, replica, base, base + S, base + 2 * S);
  if ((rc = launch_check(ctx))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t len = (size_t)(max_voted - lo + 1);
  std::vector<int32_t> vr(len), vv(len);
  HIPCHK(ctx, hipMemcpy(vr.data(), base + lo, len * 4, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(vv.data(), base + S + lo, len * 4, hipMemcpyDeviceToHost));
  int32_t k = 0;
  for (size_t j = 0; j < len; ++j) {
    if (vr[j] < 0) continue;  // no vote in the slot (or another group's slot)
    if (k < cap) slot[k] = (int32_t)(lo + (int64_t)j), vote_round[k] = vr[j], vote_value[k] = vv[j];
    ++k;
  }
  *count = k;
  return FPX_OK;
}

int32_t fpx_acceptor_phase1b_info_all_dev(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* d_acceptor_masks, int64_t cap,
                                          int64_t* d_offsets, int32_t* d_slot, int32_t* d_vote_round, int32_t* d_vote_value,
                                          int64_t* d_totals) {
  if (!p1i_args_ok(ctx, cap, d_offsets, d_slot, d_vote_round, d_vote_value, d_totals)) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (the scan is [watermark, S), never bounded by max_voted: a pending fold stays pending)
  return enqueue_p1i(ctx, chosen_watermark, d_acceptor_masks, cap, d_offsets, d_slot, d_vote_round, d_vote_value, d_totals);
}

int32_t fpx_acceptor_phase1b_info_all(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* acceptor_masks, int64_t cap,
                                      int64_t* offsets, int32_t* slot, int32_t* vote_round, int32_t* vote_value, int64_t* count) {
  if (!p1i_args_ok(ctx, cap, offsets, slot, vote_round, vote_value, count)) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);
  return host_p1i(ctx, chosen_watermark, acceptor_masks, nullptr, cap, offsets, slot, vote_round, vote_value, count);
}

int32_t fpx_acceptor_phase1(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, const uint64_t* target_masks,
                            uint64_t* promised_bits, uint64_t* nack_bits, int64_t cap, int64_t* offsets, int32_t* slot,
                            int32_t* vote_round, int32_t* vote_value, int64_t* count) {
  if (!p1i_args_ok(ctx, cap, offsets, slot, vote_round, vote_value, count) || round < 0 || round > MAX_ROUND) return FPX_EINVAL;
  DeviceGuard _dg(ctx->cfg.device);  // (enqueue_phase1a deals with a pending fold)
  const int ng = ctx->g.ngroups;
  const size_t words = (size_t)ng * 4;
  int rc;
  // the promised bits (the info pass's masks), the nack bits, the targets: outside the staging buffer, which is host_p1i's
  if ((rc = grow(ctx, &ctx->d_scratch, 3 * words * 8))) return rc;
  uint64_t *d_prom = (uint64_t*)ctx->d_scratch.p, *d_nack = d_prom + words, *d_tgt = d_nack + words;
  if (target_masks) HIPCHK(ctx, hipMemcpyAsync(d_tgt, target_masks, words * 8, hipMemcpyHostToDevice, ctx->stream));
  // the reply bits of the groups nobody addressed (the Phase1a kernels write an addressed group's in full)
  HIPCHK(ctx, hipMemsetAsync(d_prom, 0, words * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_nack, 0, words * 8, ctx->stream));
  for (int grp = 0; grp < ng; ++grp) {
    if (target_masks) {
      const uint64_t* t = target_masks + (size_t)grp * 4;
      bool any = false;
      for (int w = 0; w < 4; ++w) any = any || (t[w] & ctx->g.member[w]) != 0;
      if (!any) continue;  // nobody of the group is addressed
    }
    if ((rc = enqueue_phase1a(ctx, grp, round, chosen_watermark, target_masks ? d_tgt + (size_t)grp * 4 : nullptr,
                              d_prom + (size_t)grp * 4, d_nack + (size_t)grp * 4)))
      return rc;
  }
  rc = host_p1i(ctx, chosen_watermark, nullptr, d_prom, cap, offsets, slot, vote_round, vote_value, count);  // (synchronises)
  // the reply bits last, straight into the caller's arrays
  if (promised_bits) HIPCHK(ctx, hipMemcpyAsync(promised_bits, d_prom, words * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (nack_bits) HIPCHK(ctx, hipMemcpyAsync(nack_bits, d_nack, words * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return rc;
}

// ---- multi-GPU: RCCL behind the C ABI ------------------------------------------------------------------
static RcclApi* rccl_bind();
// bound once per process, also when two contexts create their communicators from two threads (a function-local
// static's initialiser runs exactly once)
static RcclApi* rccl() {
  static RcclApi* const bound = rccl_bind();
  return bound;
}
static RcclApi* rccl_bind() {
  static RcclApi api;
  void* h = nullptr;
  const char* env = getenv("FPX_RCCL_LIB");
  if (env && *env) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
  // an RCCL that is already mapped (PyTorch's bundled copy) wins over loading a second one
  const char* loaded[] = {"librccl.so", "librccl.so.1"};
  for (size_t i = 0; !h && i < 2; ++i) h = dlopen(loaded[i], RTLD_NOW | RTLD_NOLOAD);
  const char* fresh[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (size_t i = 0; !h && i < 3; ++i) h = dlopen(fresh[i], RTLD_NOW | RTLD_GLOBAL);
  if (!h) return nullptr;
  auto sym = [&](const char* name) { return dlsym(h, name); };
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
  api.ReduceScatter = reinterpret_cast<decltype(api.ReduceScatter)>(sym("ncclReduceScatter"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
  api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(sym("ncclAllReduce"));
  api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
  api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
  if (!api.GroupStart || !api.GroupEnd) api.GroupStart = api.GroupEnd = nullptr;
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.ReduceScatter || !api.AllGather) return nullptr;
  api.lib = h;
  return &api;
}

#define RCCLCHK(ctx, expr)                 \
  do {                                     \
    int _r = (expr);                       \
    if (_r != 0) {                         \
      if (ctx) (ctx)->last_rccl = _r;      \
      return FPX_ERCCL;                    \
    }                                      \
  } while (0)

int32_t fpx_comm_unique_id(uint8_t id[FPX_COMM_ID_BYTES]) {
  if (!id) return FPX_EINVAL;
  RcclApi* r = rccl();
  if (!r) return FPX_ERCCL;
  RcclUniqueId u;
  if (r->GetUniqueId(&u) != 0) return FPX_ERCCL;
  memcpy(id, u.internal, FPX_COMM_ID_BYTES);
  return FPX_OK;
}

int32_t fpx_comm_create(fpx_ctx* ctx, const uint8_t id[FPX_COMM_ID_BYTES], int32_t rank, int32_t world) {
  DeviceGuard _dg(ctx);
  if (!ctx || !id || world < 1 || rank < 0 || rank >= world || ctx->comm) return FPX_EINVAL;
  RcclApi* r = rccl();
  if (!r) return FPX_ERCCL;
  RcclUniqueId u;
  memcpy(u.internal, id, FPX_COMM_ID_BYTES);
  RcclComm c = nullptr;
  RCCLCHK(ctx, r->CommInitRank(&c, world, u, rank));  // binds to the current device = the context's
  ctx->comm = c;
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  return FPX_OK;
}

int32_t fpx_comm_destroy(fpx_ctx* ctx) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  if (!ctx->comm) return FPX_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  RcclApi* r = rccl();
  if (r) RCCLCHK(ctx, r->CommDestroy(ctx->comm));
  ctx->comm = nullptr;
  ctx->comm_rank = 0, ctx->comm_world = 1;
  return FPX_OK;
}

int32_t fpx_comm_info(fpx_ctx* ctx, int32_t* rank, int32_t* world) {
  if (!ctx) return FPX_EINVAL;
  if (rank) *rank = ctx->comm_rank;
  if (world) *world = ctx->comm_world;
  return FPX_OK;
}

int32_t fpx_last_rccl_error(fpx_ctx* ctx) { return ctx ? ctx->last_rccl : 0; }

int32_t fpx_profile_read_collective(fpx_ctx* ctx, int32_t* launches, double* total_ms) {
  DeviceGuard _dg(ctx);
  if (!ctx) return FPX_EINVAL;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  double sum = 0;
  for (size_t i = 0; i + 1 < ctx->cev_used; i += 2) {
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->cev[i], ctx->cev[i + 1]));
    sum += ms;
  }
  if (launches) *launches = (int32_t)(ctx->cev_used / 2);
  if (total_ms) *total_ms = sum;
  ctx->cev_used = 0;
  return FPX_OK;
}

int32_t fpx_phase2_replica_sharded_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                                       const int32_t* d_value_id, const uint64_t* d_target_mask, uint8_t* d_chosen,
                                       int32_t* d_chosen_round, int32_t* d_chosen_value, int32_t* d_nack_round) {
  DeviceGuard _dg(ctx);
  if (!ctx || n < 0) return FPX_EINVAL;
  const int world = ctx->comm_world, rank = ctx->comm_rank;
  if (n % world) return FPX_EINVAL;
  if (n == 0) return FPX_OK;
  const int per = n / world, lo = rank * per;
  int rc;
  if ((rc = grow(ctx, &ctx->d_part, (size_t)n * 32))) return rc;
  if (ctx->comm && (rc = grow(ctx, &ctx->d_mine, (size_t)per * 32))) return rc;
  uint64_t* part = (uint64_t*)ctx->d_part.p;
  // K1: my acceptor columns vote on every slot of the batch; partial bitmaps (bits in my range only) to HBM
  Batch b = batch_of(n, d_slot, d_round, d_value_id, d_target_mask);
  b.vote_bits = part, b.nack_round = d_nack_round;
  if ((rc = enqueue_phase2(ctx, b, false, RunOpts{}))) return rc;
  const uint64_t* mine = part + (size_t)lo * 4;
  if (ctx->comm) {  // also on a communicator of one rank: the same call path, RCCL copies
    // the exchange step: sum (== OR) of the partial bitmaps, scattered so that I receive my slots' rows
    RcclApi* r = rccl();
    if (!r) return FPX_ERCCL;
    const bool prof = ctx->profiling && ctx->cev_used + 2 <= ctx->cev.size();
    if (prof) HIPCHK(ctx, hipEventRecord(ctx->cev[ctx->cev_used], ctx->stream));
    RCCLCHK(ctx, r->ReduceScatter(part, ctx->d_mine.p, (size_t)per * 4, RCCL_UINT64, RCCL_SUM, ctx->comm, ctx->stream));
    if (prof) {
      HIPCHK(ctx, hipEventRecord(ctx->cev[ctx->cev_used + 1], ctx->stream));
      ctx->cev_used += 2;
    }
    mine = (const uint64_t*)ctx->d_mine.p;
    // a Nack from ANY rank's acceptors reaches the caller (Leader.handleNack reacts to the largest round, Leader.scala:
    // 672-697): max over the ranks, 4 B per slot more on the wire
    if (d_nack_round && world > 1) {
      if (!r->AllReduce) return FPX_ERCCL;
      RCCLCHK(ctx, r->AllReduce(d_nack_round, d_nack_round, (size_t)n, RCCL_INT32, RCCL_MAX, ctx->comm, ctx->stream));
    }
  }
  // ProxyLeader.handlePhase2a bookkeeping + handlePhase2b for my slice of the slots; K1's validation pass
  // covered the whole batch (slots distinct), so the slice needs none
  const RunOpts covered{RunOpts::CUT_ON_HOST};
  Batch o = batch_of(per, d_slot + lo, d_round + lo, d_value_id + lo);
  if ((rc = enqueue_open(ctx, o, covered))) return rc;
  Batch t = batch_of(per, d_slot + lo, d_round + lo, nullptr);
  t.vote_bits = const_cast<uint64_t*>(mine);
  t.chosen = d_chosen, t.chosen_round = d_chosen_round, t.chosen_value = d_chosen_value;
  return enqueue_tally(ctx, t, covered);
}

int32_t fpx_comm_allgather_chosen_dev(fpx_ctx* ctx, int32_t n_local, const uint8_t* d_chosen,
                                      const int32_t* d_chosen_round, const int32_t* d_chosen_value,
                                      uint8_t* d_all_chosen, int32_t* d_all_round, int32_t* d_all_value) {
  DeviceGuard _dg(ctx);
  if (!ctx || n_local < 0) return FPX_EINVAL;
  if (n_local == 0) return FPX_OK;
  if (ctx->comm_world == 1) {  // degenerate: a device copy
    if (d_chosen && d_all_chosen) HIPCHK(ctx, hipMemcpyAsync(d_all_chosen, d_chosen, (size_t)n_local, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_chosen_round && d_all_round) HIPCHK(ctx, hipMemcpyAsync(d_all_round, d_chosen_round, (size_t)n_local * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_chosen_value && d_all_value) HIPCHK(ctx, hipMemcpyAsync(d_all_value, d_chosen_value, (size_t)n_local * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return FPX_OK;
  }
  RcclApi* r = rccl();
  if (!r || !ctx->comm) return FPX_ERCCL;
  const bool prof = ctx->profiling && ctx->cev_used + 2 <= ctx->cev.size();
  if (prof) HIPCHK(ctx, hipEventRecord(ctx->cev[ctx->cev_used], ctx->stream));
  // the three arrays of the Chosen records travel as ONE group: one launch and one ring set-up instead of three
  // (ncclGroupStart / ncclGroupEnd; an RCCL without them gets three calls)
  if (r->GroupStart) RCCLCHK(ctx, r->GroupStart());
  int grc = 0;
  if (d_chosen && d_all_chosen) grc = r->AllGather(d_chosen, d_all_chosen, (size_t)n_local, RCCL_UINT8, ctx->comm, ctx->stream);
  if (!grc && d_chosen_round && d_all_round) grc = r->AllGather(d_chosen_round, d_all_round, (size_t)n_local, RCCL_INT32, ctx->comm, ctx->stream);
  if (!grc && d_chosen_value && d_all_value) grc = r->AllGather(d_chosen_value, d_all_value, (size_t)n_local, RCCL_INT32, ctx->comm, ctx->stream);
  if (r->GroupEnd) {  // (always closed, also after a failed call inside the group)
    const int erc = r->GroupEnd();
    if (!grc) grc = erc;
  }
  RCCLCHK(ctx, grc);
  if (prof) {
    HIPCHK(ctx, hipEventRecord(ctx->cev[ctx->cev_used + 1], ctx->stream));
    ctx->cev_used += 2;
  }
  return FPX_OK;
}

int32_t fpx_state_digest(fpx_ctx* ctx, uint64_t out[8]) {
  DeviceGuard _dg(ctx);
  if (!ctx || !out) return FPX_EINVAL;
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  uint64_t* d = (uint64_t*)ctx->d_scratch.p;
  if ((rc = flush_promises(ctx))) return rc;
  HIPCHK(ctx, hipMemsetAsync(d, 0, 64, ctx->stream));
  const Geom& g = ctx->g;
  const int big = ctx->num_cus * 16;
  const size_t n4 = (size_t)g.S * (size_t)(g.RS / 4);
  const int gc = (int)std::max<size_t>(1, std::min<size_t>((n4 + 255) / 256, (size_t)big));
  hipLaunchKernelGGL(k_digest_cells, dim3(gc), dim3(256), 0, ctx->stream, g, ctx->st, ctx->st.vote_round, g.VS, 0, d + 0);
  hipLaunchKernelGGL(k_digest_cells, dim3(gc), dim3(256), 0, ctx->stream, g, ctx->st, ctx->st.vote_value, g.VS, 1, d + 1);
  if (ctx->st.ballot) hipLaunchKernelGGL(k_digest_cells, dim3(gc), dim3(256), 0, ctx->stream, g, ctx->st, ctx->st.ballot, g.RS, -1, d + 2);
  const int nsc = g.ngroups * g.R;
  const int gs = std::max(1, std::min((nsc + 255) / 256, big));
  hipLaunchKernelGGL(k_digest_1d, dim3(gs), dim3(256), 0, ctx->stream, ctx->st.promised, nsc, d + 3);
  hipLaunchKernelGGL(k_digest_1d, dim3(gs), dim3(256), 0, ctx->stream, ctx->st.max_voted, nsc, d + 4);
  const int gt = std::max(1, std::min((g.S + 255) / 256, big));
  hipLaunchKernelGGL(k_digest_tally, dim3(gt), dim3(256), 0, ctx->stream, g, ctx->st, d + 5);
  hipLaunchKernelGGL(k_digest_log, dim3(gt), dim3(256), 0, ctx->stream, g, ctx->st, d + 6);
  if (ctx->rt[0].key) {
    const RangeTable& rt = ctx->rt[ctx->rt_cur];
    hipLaunchKernelGGL(k_digest_ranges, dim3(std::max(1, std::min((rt.cap + 255) / 256, big))), dim3(256), 0, ctx->stream, rt,
                       g.num_groups * 4, d + 7);
  }
  if ((rc = launch_check(ctx))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

int32_t fpx_ballot_summary_audit(fpx_ctx* ctx, int64_t out[3]) {
  DeviceGuard _dg(ctx);
  if (!ctx || !out || !ctx->g.per_slot) return FPX_EINVAL;
  if (!ctx->st.ballot_sum) {  // rows of at most 128 cells: no summaries, every row counts as mixed
    out[0] = 0, out[1] = ctx->g.S, out[2] = 0;
    return FPX_OK;
  }
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  unsigned long long* d = (unsigned long long*)ctx->d_scratch.p;
  HIPCHK(ctx, hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), ctx->stream));
  const Geom& g = ctx->g;
  const dim3 grid(ctx->num_cus * 8);
  if (g.R > 32) hipLaunchKernelGGL(k_ballot_audit<64>, grid, dim3(256), 0, ctx->stream, g, ctx->st, d);
  else if (g.R > 4) hipLaunchKernelGGL(k_ballot_audit<8>, grid, dim3(256), 0, ctx->stream, g, ctx->st, d);
  else hipLaunchKernelGGL(k_ballot_audit<1>, grid, dim3(256), 0, ctx->stream, g, ctx->st, d);
  if ((rc = launch_check(ctx))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

int32_t fpx_vote_summary_audit(fpx_ctx* ctx, int64_t out[3]) {
  DeviceGuard _dg(ctx);
  if (!ctx || !out) return FPX_EINVAL;
  int rc;
  if ((rc = grow(ctx, &ctx->d_scratch, 128))) return rc;
  unsigned long long* d = (unsigned long long*)ctx->d_scratch.p;
  HIPCHK(ctx, hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_vote_audit, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, ctx->g, ctx->st, d);
  if ((rc = launch_check(ctx))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FPX_OK;
}

int32_t fpx_read_tally(fpx_ctx* ctx, int32_t slot, int32_t* num_entries, int32_t* rounds, int32_t* states,
                       int32_t* values, uint64_t* vote_bits) {
  DeviceGuard _dg(ctx);
  if (!ctx || slot < 0 || slot >= ctx->g.S) return FPX_EINVAL;
  const int wp = ctx->g.wp;
  uint32_t keys[8];
  int32_t vals[8];
  uint64_t bits[32];
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t prow = host_phys_slot(ctx->g, slot);
  HIPCHK(ctx, hipMemcpy(keys, ctx->st.pl_key + prow * wp, (size_t)wp * 4, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(vals, ctx->st.pl_value + prow * wp, (size_t)wp * 4, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(bits, ctx->st.pl_bits + prow * wp * 4, (size_t)wp * 32, hipMemcpyDeviceToHost));
  int cnt = 0;
  for (int w = 0; w < ctx->g.ways; ++w) {
    if (keys[w] == 0 || (keys[w] & KEY_RANGE)) continue;  // range tallies are not per-slot tallies
    const bool done = keys[w] & KEY_DONE;
    if (rounds) rounds[cnt] = (int32_t)((keys[w] & KEY_ROUND_MASK) - 1u);
    if (states) states[cnt] = done ? 1 : 0;
    // a Done entry has dropped its Pending payload (ProxyLeader.scala:256)
    if (values) values[cnt] = done ? -1 : vals[w];
    if (vote_bits)
      for (int k = 0; k < 4; ++k) vote_bits[(size_t)cnt * 4 + k] = done ? 0ull : bits[w * 4 + k];
    ++cnt;
  }
  if (num_entries) *num_entries = cnt;
  return FPX_OK;
}

}  // extern "C"
