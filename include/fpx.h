/*
 * fpx.h -- C ABI of libfpx: the MI355X (gfx950) Phase-2 accept / quorum-tally engine.
 *
 * This is the drop-in boundary for ONE hot path of mwhittaker/frankenpaxos:
 *
 *   a1  multipaxos.Acceptor.handlePhase2a     shared/src/main/scala/frankenpaxos/multipaxos/Acceptor.scala:184-220
 *   a2  mencius.Acceptor.handlePhase2a        shared/src/main/scala/frankenpaxos/mencius/Acceptor.scala:202-235
 *   a3  multipaxos.ProxyLeader.handlePhase2b  shared/src/main/scala/frankenpaxos/multipaxos/ProxyLeader.scala:217-258
 *   a4  mencius.ProxyLeader.handlePhase2b     shared/src/main/scala/frankenpaxos/mencius/ProxyLeader.scala:305-353
 *   a5  quorums.*.isWriteQuorum / isSuperSetOfWriteQuorum
 *                                             shared/src/main/scala/frankenpaxos/quorums/{SimpleMajority,Grid,UnanimousWrites}.scala
 *   a6  multipaxos.ProxyLeader.handlePhase2a  shared/src/main/scala/frankenpaxos/multipaxos/ProxyLeader.scala:175-215
 *   a7  roundsystem.ClassicRoundRobin         shared/src/main/scala/frankenpaxos/roundsystem/RoundSystem.scala:60-87
 *   a8  simulator.FakeTransport (delivery)    shared/src/main/scala/frankenpaxos/FakeTransport.scala:89-159
 *
 * The reference has no FFI of its own (it is pure Scala); the seam is the Actor/Transport trait
 * surface.  A JNI shim marshals one event-loop tick worth of Phase2a / Phase2b
 * protobuf messages into the struct-of-arrays batches below and calls these entry points once per
 * batch.  Everything is plain pointers + sizes; no torch / HIP types appear in a signature (a HIP
 * stream crosses as void*).
 *
 * Conventions
 *   - Every function returns an int32 status (FPX_OK == 0).  FPX_EINVAL corresponds to a Scala
 *     require(...) failure; FPX_EFATAL_UNKNOWN_SLOTROUND to logger.fatal in
 *     ProxyLeader.handlePhase2b (ProxyLeader.scala:220-225).  A stale round is NOT an error: it
 *     produces a Nack exactly as in the reference.
 *   - A context is NOT thread-safe: one caller thread per context, mirroring "All Transport
 *     implementations MUST be single-threaded" (shared/src/main/scala/frankenpaxos/Transport.scala:37-39).
 *   - Entry points without a suffix take HOST pointers, are synchronous, and accept ANY batch: the
 *     library splits it into device "runs" so that the result equals message-at-a-time delivery in
 *     array order.  Entry points ending in _dev take DEVICE pointers (resident in HBM), enqueue on
 *     the context's stream and return immediately; the batch must already satisfy the run contract
 *     (below) -- a violation is detected on the device, nothing is applied, and the next fpx_sync()
 *     returns FPX_EORDER.
 *   - Run contract (one kernel launch): (1) slots in the batch are pairwise distinct; (2) in
 *     FPX_BALLOT_ACCEPTOR mode all messages addressed to one acceptor group carry the same round
 *     (different groups may be in different rounds).  Under (2) the acceptor's running-max `round`
 *     (Acceptor.scala:95,204) seen by message i equals max(round at batch start, round[i]) for every
 *     acceptor, which is what lets a batch be evaluated data-parallel and still be bit-exact.  A
 *     proxy leader's event-loop tick satisfies both in steady state; the host entry points cut any
 *     other batch at the offending message and launch the pieces back to back.
 *   - Bitmaps: one message's set of acceptors is 4 x uint64 (256 bits); bit j of the 256-bit
 *     little-endian integer is acceptor index j of the slot's acceptor group (for a Grid:
 *     j = row * grid_cols + col, row = groupIndex, col = acceptorIndex).
 *   - value_id is an int32 standing in for CommandBatchOrNoop (FPX_NOOP == -1 is Noop).
 */
#ifndef FPX_H
#define FPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPX_VERSION 100

#define FPX_MAX_REPLICAS 256
#define FPX_MASK_WORDS 4
#define FPX_NOOP (-1)

/* status codes.  What a non-OK status says about the state:
 *   FPX_EINVAL / FPX_EORDER   raised by the validation pass BEFORE anything of the batch is applied: the
 *                             batch -- and every later _dev call up to the next fpx_sync -- applied nothing.
 *   FPX_ECAPACITY             per message: that message's tally could not be opened, so it was neither
 *                             recorded nor forwarded to the acceptors (as if the proxy leader had never
 *                             received it); every other message of the batch was applied in full, acceptor
 *                             rounds and maxVotedSlot included.  The reference has no such limit
 *                             (ProxyLeader.states grows forever): free ways with fpx_proxy_forget or raise
 *                             tally_ways and resend the message.
 *   FPX_EFATAL_UNKNOWN_SLOTROUND  per message (the reference process would have died in logger.fatal): that
 *                             Phase2b was dropped, the others were applied.
 *   FPX_EHIP / FPX_ENOMEM     the HIP runtime failed; the context should be destroyed.
 * fpx_error_detail names the first offending message. */
enum {
  FPX_OK = 0,
  FPX_EINVAL = 1,                   /* == Scala require(...) / IllegalArgumentException            */
  FPX_EFATAL_UNKNOWN_SLOTROUND = 2, /* == logger.fatal, ProxyLeader.scala:220-225                    */
  FPX_EHIP = 3,                     /* a HIP runtime call failed (fpx_last_hip_error has the code)   */
  FPX_ENODEVICE = 4,                /* no gfx950 device / HIP runtime: there is NO CPU fallback      */
  FPX_ECAPACITY = 5,                /* more than tally_ways live (slot, round) tallies for one slot  */
  FPX_EORDER = 6,                   /* a _dev batch violated the run contract; nothing was applied   */
  FPX_ENOMEM = 7,
  FPX_ERCCL = 8,                    /* an RCCL call failed / RCCL is not loadable (fpx_last_rccl_error)  */
  FPX_EFATAL_PROTOCOL = 9           /* a logger.fatal / logger.check of the reference would have fired for a
                                       message (EPaxos: transitionToAcceptPhase on a committed instance or
                                       below an entry's ballot, Replica.scala:740-757): that message was not
                                       applied, the others were                                             */
};

typedef enum {
  FPX_Q_THRESHOLD = 0,       /* |X| >= f+1             ProxyLeader.scala:238 (non-flexible)          */
  FPX_Q_SIMPLE_MAJORITY = 1, /* |X| >= n/2+1           SimpleMajority.scala:30,41-49                 */
  FPX_Q_GRID = 2,            /* every row intersects X Grid.scala:43-50                              */
  FPX_Q_UNANIMOUS = 3        /* X == members           UnanimousWrites.scala:44-51                   */
} fpx_quorum_kind;

typedef enum {
  /* one promised `round` per acceptor, shared by all its slots: multipaxos/mencius Acceptor
   * (Acceptor.scala:95).  Faithful model. */
  FPX_BALLOT_ACCEPTOR = 0,
  /* one ballot per (slot, acceptor) cell, stored in HBM next to voteRound / voteValue: the
   * per-instance ballot of epaxos.Replica.handleAccept (epaxos/Replica.scala:1421-1510) and the
   * "generalised ballot[S x R]" model of SURVEY.md section 8(d). */
  FPX_BALLOT_PER_SLOT = 1
} fpx_ballot_mode;

/* flags */
#define FPX_F_TRUSTED 1u /* _dev entry points skip the run-contract validation pass (caller guarantees it) */
/* Hint: target masks are scattered subsets of the group -- the reference's thrifty default, a random f+1
 * of 2f+1 (ProxyLeader.scala:190-191).  K1 / K3 launches that carry target masks then write partially
 * voted 16-byte cells by read-modify-write instead of 4-byte stores.  Results are identical either way. */
#define FPX_F_SCATTERED_TARGETS 2u
/* Without that hint, on 256-cell rows of one acceptor group (R = 253 .. 256, threshold / majority / unanimous quorums),
 * launches that carry target masks run as TWO kernels: chunks of up to 64 messages that all go to a RUN of neighbouring
 * acceptors -- positions [start, start + len) of the row, cyclically, start a multiple of 16, len <= 128: what a proxy
 * leader sends that rotates a window of f + 1 acceptors over the group instead of shuffling (any f + 1 will do,
 * ProxyLeader.scala:190-191; jni/Native.scala's GpuProxyLeader does) -- of rows nobody voted in yet are walked two
 * rows per wavefront step (a row costs the same instructions whatever it moves, so half a row at a time ran at the
 * dense rate: 3.0e9 slots/s; now 4.4e9), every other chunk by the row-at-a-time walk behind it.  The hint skips the
 * first kernel.  Results are identical either way (FPX_NO_PACKED_RUNS in the environment switches the first kernel off). */
/* Mencius contexts (num_leader_groups L > 1, num_slots a multiple of L, num_replicas <= 32) keep the per-slot rows of the cell arrays and
 * tally tables LEADER-GROUP-MAJOR in HBM -- slot s lives in row (s % L) * (S / L) + s / L -- so that what one leader
 * group does (a noop range = every L-th slot; its batch of Phase2as in slot order) touches neighbouring rows and
 * every 128-byte line leaves the GPU whole.  A launch is fastest as the leader groups' batches back to back; one batch
 * in slot order across the leader groups is walked column by column by the kernel and is still faster than on
 * slot-ordered rows (profiles/r03_cfg5.md).  This flag keeps rows in slot order (round 2's layout).  Results are
 * identical either way; only speed differs. */
#define FPX_F_SLOT_MAJOR_ROWS 4u

typedef struct {
  int32_t num_slots;         /* S: log window held in HBM; slots are 0 .. S-1                          */
  int32_t num_replicas;      /* R: acceptors per acceptor group, 1 .. 256                               */
  int32_t num_groups;        /* acceptor groups per leader group; slot -> group as below                */
  int32_t num_leader_groups; /* 1 for MultiPaxos.  Mencius: leader group = slot % num_leader_groups,
                                acceptor group = (slot / num_leader_groups) % num_groups
                                (mencius/ProxyLeader.scala:231-234); group id = lg * num_groups + ag     */
  int32_t f;                 /* FPX_Q_THRESHOLD: quorum size f+1                                         */
  int32_t quorum_kind;       /* fpx_quorum_kind                                                          */
  int32_t grid_rows, grid_cols; /* FPX_Q_GRID: rows * cols == num_replicas                               */
  int32_t num_leaders;       /* ClassicRoundRobin(num_leaders): Nack routing, Acceptor.scala:197         */
  int32_t ballot_mode;       /* fpx_ballot_mode                                                          */
  int32_t tally_ways;        /* live (slot, round) tallies kept per slot, 1 .. 8 (ProxyLeader.states is
                                keyed by SlotRound, ProxyLeader.scala:87,135)                            */
  int32_t replica_base;      /* multi-GPU replica-axis sharding: this context owns acceptors
                                [replica_base, replica_base + num_replicas) of a group of
                                replicas_total acceptors; multiple of 4; 0 when not sharded             */
  int32_t replicas_total;    /* 0 => num_replicas.  Quorum predicates are over replicas_total.          */
  int32_t device;            /* HIP device ordinal.  Every entry point makes it current for the duration
                                of the call and restores the caller's device, so contexts on several GPUs
                                can be driven from one thread                                              */
  uint32_t flags;            /* FPX_F_*                                                                  */
} fpx_config;

typedef struct fpx_ctx fpx_ctx;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int32_t fpx_version(void);
const char* fpx_strerror(int32_t status);
/* validates the config exactly like Config.checkValid-style require()s (FPX_EINVAL), no GPU needed */
int32_t fpx_config_check(const fpx_config* cfg);
/* allocates HBM state: acceptors start with round = -1 and no votes (Acceptor.scala:95-104),
 * the proxy leader with no tallies (ProxyLeader.scala:135). */
int32_t fpx_create(const fpx_config* cfg, fpx_ctx** out);
int32_t fpx_destroy(fpx_ctx* ctx);
/* re-initialises all state to the freshly-created state (device memset, async on the stream) */
int32_t fpx_reset(fpx_ctx* ctx);
/* hip_stream is a hipStream_t passed through as it is: NULL is the device's default (null) stream --
 * which is what torch.cuda.current_stream().cuda_stream is unless the caller switched streams --
 * and FPX_STREAM_OWN selects the context's private stream (the state after fpx_create).  The _dev
 * entry points enqueue on this stream: device inputs must be produced on it (or ordered before it). */
#define FPX_STREAM_OWN ((void*)(intptr_t)-1)
int32_t fpx_set_stream(fpx_ctx* ctx, void* hip_stream);
/* waits for the stream; returns the sticky device status of the _dev calls since the last sync
 * (FPX_OK, FPX_EORDER, FPX_ECAPACITY, FPX_EFATAL_UNKNOWN_SLOTROUND, FPX_EINVAL) and clears it */
int32_t fpx_sync(fpx_ctx* ctx);
/* index / slot / round of the first offending message of the last non-OK status */
int32_t fpx_error_detail(fpx_ctx* ctx, int32_t* index, int32_t* slot, int32_t* round);
int32_t fpx_last_hip_error(fpx_ctx* ctx);
/* HBM bytes held by the context */
int64_t fpx_device_bytes(fpx_ctx* ctx);
/* How the cell arrays (Acceptor.states of every acceptor, multipaxos/Acceptor.scala:98) were placed in HBM by fpx_create:
 * out[0] = 1 if the slab is built from 1 GiB physical chunks paired by measurement (vote_round's and vote_value's chunk of
 * a gigabyte of rows must be a pair the chip writes side by side at the fast rate; contexts of 2 GiB and more with groups
 * of 61+ acceptors), 0 if it is one allocation; out[1] = gigabyte windows probed; out[2..4] = min / median / max over the
 * windows of the hot access pattern's time on half a window, in ms (0 when nothing was probed).  Diagnostics only:
 * results never depend on the placement.  FPX_PLACEMENT_CHUNKS=0 in the environment keeps one allocation. */
int32_t fpx_placement_stats(fpx_ctx* ctx, float out[5]);
/* What the placement search of fpx_create cost: probes run, decisions taken WITHOUT a probe because the search's budget
 * was spent, and the wall clock of the search in ms.  The budget is FPX_PLACEMENT_BUDGET_MS in the environment (default
 * 300 ms; 0 = no probing at all: the slab is built from the chunks in allocation order): once it is spent every remaining
 * decision takes its first candidate, so N ranks creating contexts at once cannot stretch fpx_create without bound.  Any
 * of the three pointers may be NULL.  Diagnostics only. */
int32_t fpx_placement_search(fpx_ctx* ctx, int32_t* probes, int32_t* unprobed, float* ms);
/* the configuration the context was created with (replicas_total filled in): a binding sizes its buffers from the
 * handle, not from what its caller says the handle is */
int32_t fpx_get_config(fpx_ctx* ctx, fpx_config* out);
/* Page-locked host memory for the host-pointer entry points: batches that live in it cross PCIe by DMA at
 * link rate instead of through the runtime's pageable staging copies.  A JVM caller wraps the region in
 * a direct ByteBuffer (JNI NewDirectByteBuffer), the counterpart of the Netty direct buffers the
 * reference's transports hand to the handlers.  Any other host pointer stays legal, only slower. */
int32_t fpx_host_alloc(int64_t bytes, void** out);
int32_t fpx_host_free(void* p);
/* Kernel timing for roofline accounting: while enabled, every K1 / K3 call brackets its dominant
 * kernel (k_phase2) with HIP events on the context's stream.  fpx_profile_read waits for the stream
 * and returns the number of bracketed launches since the last read and the sum of their durations. */
int32_t fpx_profile_enable(fpx_ctx* ctx, int32_t on);
int32_t fpx_profile_read(fpx_ctx* ctx, int32_t* launches, double* total_ms);
/* the same read launch by launch: the durations of the first `cap` timed launches since the last read, in order, into
 * ms_out; *launches = how many there were (the variance of one kernel over the log's windows: profiles/r05_placement.md) */
int32_t fpx_profile_read_launches(fpx_ctx* ctx, int32_t cap, float* ms_out, int32_t* launches);

/* ---- a7: roundsystem.ClassicRoundRobin (RoundSystem.scala:60-87); pure host scalars ----------- */
int32_t fpx_round_leader(int32_t num_leaders, int32_t round);                         /* :63     */
int32_t fpx_next_classic_round(int32_t num_leaders, int32_t leader_index, int32_t round); /* :66-81 */

/* ---- a5: quorum predicates on the device ----------------------------------------------------- */
/* Evaluates isWriteQuorum (strict = 1: FPX_EINVAL if a bit outside the member set is present, the
 * require() of SimpleMajority.scala:42 / Grid.scala:44 / UnanimousWrites.scala:45) or
 * isSuperSetOfWriteQuorum (strict = 0: foreign bits ignored) for n node sets; nodes is n x 4 words,
 * out is n bytes (host pointers).  Only the quorum fields of cfg are read.  Runs the same device
 * function the tally kernels use. */
int32_t fpx_quorum_eval(const fpx_config* cfg, int32_t n, const uint64_t* nodes, int32_t strict,
                        uint8_t* out);
int32_t fpx_is_write_quorum(const fpx_config* cfg, const uint64_t nodes[4], int32_t strict,
                            uint8_t* out);
/* isReadQuorum / isSuperSetOfReadQuorum with the same conventions (SimpleMajority.scala:41-47,
 * Grid.scala:36-41,52-53, UnanimousWrites.scala:36-42,53-54) */
int32_t fpx_read_quorum_eval(const fpx_config* cfg, int32_t n, const uint64_t* nodes, int32_t strict,
                             uint8_t* out);

/* ---- a1/a2 (K1): acceptors handle Phase2a -------------------------------------------------------
 * Delivers Phase2a(slot[i], round[i], value_id[i]), i = 0..n-1 in array order, to the acceptors of
 * the slot's group selected by target_mask (n x 4 words; NULL = every acceptor of the group).  Per
 * targeted acceptor (Acceptor.scala:192-219): round[i] < its round -> Nack(its round); otherwise
 * its round := round[i], states[slot] := (round[i], value_id[i]), maxVotedSlot := max(.., slot),
 * Phase2b.  Outputs (each may be NULL): vote_bits n x 4 words = acceptors that sent Phase2b;
 * nack_bits n x 4 words = acceptors that sent Nack; nack_round n ints = the largest round carried
 * by a Nack for message i, -1 if none (the only field Leader.handleNack, Leader.scala:672-697,
 * reacts to; destination leader = fpx_round_leader(num_leaders, round[i])). */
int32_t fpx_acceptor_phase2a(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                             const int32_t* value_id, const uint64_t* target_mask,
                             uint64_t* vote_bits, uint64_t* nack_bits, int32_t* nack_round);
int32_t fpx_acceptor_phase2a_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot,
                                 const int32_t* d_round, const int32_t* d_value_id,
                                 const uint64_t* d_target_mask, uint64_t* d_vote_bits,
                                 uint64_t* d_nack_bits, int32_t* d_nack_round);

/* Phase1a (Acceptor.scala:148-182), needed so that rounds can move: acceptors of `group` selected
 * by target_mask[4] (NULL = all) with round > their round promise it (round := round), the others
 * Nack.  In FPX_BALLOT_PER_SLOT mode the promise applies to every cell of the group with
 * slot >= chosen_watermark.  promised_bits / nack_bits: 4 words each (may be NULL).
 * NOTE multipaxos uses `phase1a.round < round -> Nack` (Acceptor.scala:155), i.e. an EQUAL round is
 * promised again; that is what is implemented. */
int32_t fpx_acceptor_phase1a(fpx_ctx* ctx, int32_t group, int32_t round, int32_t chosen_watermark,
                             const uint64_t* target_mask, uint64_t* promised_bits,
                             uint64_t* nack_bits);
/* the same on device-resident arguments (each 4 words in HBM, 8-byte aligned, may be NULL), asynchronous on the context's
 * stream: a leader change in the middle of a device-resident stream costs no host round trip.  With a ballot per cell it is
 * ONE launch that writes the reply bits straight into the caller's words and does not wait for the fold of the fused step
 * before it (fpx_deferred_folds): a vote launch leaves a bound on what its fold can raise, the decision uses that
 * (csrc/fpx_kernels.hpp, k_p1a_fast) -- unless the watermark is above the smallest one handed in since the promises were
 * last flushed, which takes the three launches of rounds 2 - 5 (as does FPX_P1A_SPLIT=1 in the environment). */
int32_t fpx_acceptor_phase1a_dev(fpx_ctx* ctx, int32_t group, int32_t round, int32_t chosen_watermark,
                                 const uint64_t* d_target_mask, uint64_t* d_promised_bits,
                                 uint64_t* d_nack_bits);
/* FPX_BALLOT_PER_SLOT keeps a Phase1a that no cell is ahead of as ONE record per acceptor ("every cell from
 * the watermark on is at least `round`") instead of rewriting S x R ballots, and honours the records in the
 * vote kernels; results are identical.  This writes all outstanding records into the cells (one sweep over the
 * ballot array) and drops them, which puts the vote kernels back into their leanest form -- worth calling once
 * after the last Phase1a before a long steady stretch.  Readback and digests do it implicitly.  Asynchronous. */
int32_t fpx_acceptor_flush_promises(fpx_ctx* ctx);

/* ---- a6: ProxyLeader.handlePhase2a bookkeeping ---------------------------------------------------
 * Opens the tally Pending(phase2a, {}) for (slot[i], round[i]) (ProxyLeader.scala:213).  A (slot,
 * round) that is already known is ignored (:177-184) and reported as is_new[i] = 0.  The reference
 * picks a thrifty random quorum here (:190-196, unseeded RNG, F12 in SURVEY.md); which acceptors a
 * Phase2a goes to is the caller's target_mask in fpx_acceptor_phase2a. */
int32_t fpx_proxy_open(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                       const int32_t* value_id, uint8_t* is_new);
int32_t fpx_proxy_open_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                           const int32_t* d_value_id, uint8_t* d_is_new);

/* ---- a3/a4 (K2): ProxyLeader.handlePhase2b ----------------------------------------------------------
 * Message i carries the Phase2b's of the acceptors in vote_bits[i] for (slot[i], round[i]) (an
 * all-zero row is "no message").  Unknown (slot, round) -> FPX_EFATAL_UNKNOWN_SLOTROUND (:220-225);
 * Done -> ignored (:227-232); Pending -> votes are recorded keyed by acceptor (a duplicate vote
 * changes nothing, :237) and, when the quorum predicate holds (:238-243), Chosen(slot,
 * pending.phase2a.value) is emitted exactly once (:246-256): newly_chosen[i] = 1,
 * chosen_round[i] = round[i], chosen_value[i] = the value given to fpx_proxy_open; otherwise
 * newly_chosen[i] = 0, chosen_round[i] = chosen_value[i] = -1. */
int32_t fpx_proxy_phase2b(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                          const uint64_t* vote_bits, uint8_t* newly_chosen, int32_t* chosen_round,
                          int32_t* chosen_value);
int32_t fpx_proxy_phase2b_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                              const uint64_t* d_vote_bits, uint8_t* d_newly_chosen,
                              int32_t* d_chosen_round, int32_t* d_chosen_value);

/* The same for PER-ACCEPTOR messages, as reference acceptors send them (Acceptor.scala:211-219): message i is ONE
 * Phase2b(group_index[i], acceptor_index[i], slot[i], round[i]).  NO run contract applies: any number of messages per
 * (slot, round) in any order, several rounds of one slot, and duplicates are all allowed.  These are the outputs of
 * fpx_wire_decode_proxy_leader_inbound(_dev): kind (NULL = every message is a Phase2b; messages whose kind is not
 * FPX_WIRE_PHASE2B are skipped), group_index (NULL = 0).  The bit of a message is acceptor_index when grid_cols == 0 and
 * group_index * grid_cols + acceptor_index for a grid, as in fpx_wire_phase2b_rows.
 * Contract: the result equals fpx_wire_phase2b_rows followed by fpx_proxy_phase2b on those rows, with each row's outcome
 * reported at the index of the row's FIRST message (every other message reports newly_chosen = 0, chosen_round =
 * chosen_value = -1), and the tally state afterwards is identical -- Done entries keep their stored bits untouched.  The
 * fold runs on the device (csrc/fpx_tally_msgs.hpp: claim / gather / tally launches and an owner word per tally entry,
 * allocated by the first call: 4 bytes x num_slots x 4 or 8), with integer atomics only: results are reproducible.
 * A message whose bit lies outside the context's member set [0, replicas_total) contributes nothing: it is not looked
 * up, never reports an unknown (slot, round), and never is the "first message" of its row -- the row's outcome is at its
 * first message whose bit is a member.
 * Errors: FPX_EINVAL with NOTHING applied (the validation convention of the _dev calls: the context applies nothing up to
 * the next fpx_sync) for a bit outside 0..255, acceptor_index < 0, acceptor_index >= grid_cols for a grid, a slot
 * outside the window or a round outside 0 .. 2^30 - 2; FPX_EFATAL_UNKNOWN_SLOTROUND per message for an unknown (slot,
 * round): that message is dropped, the others are applied.  fpx_error_detail names the LOWEST offending index in both
 * cases.  n == 0 is FPX_OK.  The host form is synchronous and goes through the staging driver as a single run. */
int32_t fpx_proxy_phase2b_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                               const int32_t* acceptor_index, const int32_t* slot, const int32_t* round,
                               int32_t grid_cols, uint8_t* newly_chosen, int32_t* chosen_round, int32_t* chosen_value);
int32_t fpx_proxy_phase2b_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                   const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_round,
                                   int32_t grid_cols, uint8_t* d_newly_chosen, int32_t* d_chosen_round,
                                   int32_t* d_chosen_value);

/* Garbage collection of the proxy leader (NOT in the reference, whose ProxyLeader.states grows forever,
 * ProxyLeader.scala:135): forgets every tally -- Pending or Done -- of the slots
 * [first_slot, first_slot + count) and every noop-range tally whose range lies inside that window, so that a long-running simulation can re-propose a chosen-and-executed
 * window of the log in further rounds without exhausting tally_ways.  Acceptor state is untouched.
 * Asynchronous on the context's stream.  After it, a Phase2b for a forgotten (slot, round) is "unknown". */
int32_t fpx_proxy_forget(fpx_ctx* ctx, int32_t first_slot, int32_t count);

/* Recycling of log-window rows (NOT in the reference, whose Acceptor.states and ProxyLeader.states grow forever,
 * multipaxos/Acceptor.scala:98, ProxyLeader.scala:135): the rows [first_slot, first_slot + count) of the window
 * become fresh -- every acceptor's vote in them is dropped (voteRound = voteValue = -1, as if `states` had no
 * entry) and their tallies are forgotten (fpx_proxy_forget).  What an acceptor PROMISED stays: its scalar round
 * (FPX_BALLOT_ACCEPTOR) is untouched, and in FPX_BALLOT_PER_SLOT mode the cells keep their ballots, so a recycled
 * row never accepts a round the old row would have refused.  maxVotedSlot is left as it is (an upper bound).  A
 * host that maps an unbounded log onto the window as row = slot % num_slots calls this for the rows whose slots are
 * chosen and no longer needed before it lets the log wrap onto them (frankenpaxos_amd/jni/Native.scala, GpuPhase2).
 * Asynchronous on the context's stream. */
int32_t fpx_recycle_slots(fpx_ctx* ctx, int32_t first_slot, int32_t count);

/* ---- K3: fused step = fpx_proxy_open + fpx_acceptor_phase2a + fpx_proxy_phase2b ------------------
 * For each message in order: open (slot, round) (duplicates are ignored and NOT forwarded to the
 * acceptors, :177-184), deliver the Phase2a to the targeted acceptors (target_mask NULL = all: the
 * dense schedule of SURVEY.md section 8(d)), feed their Phase2b's to the tally.  The vote bitmap never
 * leaves the chip.  nack_round may be NULL. */
int32_t fpx_phase2_fused(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                         const int32_t* value_id, const uint64_t* target_mask, uint8_t* chosen,
                         int32_t* chosen_round, int32_t* chosen_value, int32_t* nack_round);
/* The same, asynchronous, for batches in PAGE-LOCKED host memory (fpx_host_alloc or any memory mapped into the GPU's
 * address space -- FPX_EINVAL otherwise): submit returns at once with a ticket, wait(ticket) blocks until that call's
 * outputs are in the caller's arrays and returns its status.  Up to 3 calls may be in flight (FPX_ECAPACITY: wait for
 * the oldest first); they execute in submission order.  The inputs go up by the copy engine on a stream of their own
 * into staging buffers in HBM; validation and the fused step follow on the context's stream; the vote kernel writes the
 * Chosen records (and Nack rounds) STRAIGHT into the caller's page-locked arrays -- there is no copy down.  With calls
 * submitted back to back the upload of call k + 1 hides behind the fused step of call k, which runs ~3 % longer for its
 * posted writes over PCIe (profiles/r06_host_path.md has what every other way of crossing PCIe cost the vote kernel);
 * see profiles/r06_host_path.md for the rate per 2^20 x 256 call.  A call must be ONE device run (the run
 * contract above): a violation is FPX_EORDER from wait with nothing applied -- pass that batch to fpx_phase2_fused,
 * which cuts it into runs.  After an error the calls queued behind the failed one have applied nothing either and
 * report the same status.  fpx_phase2_fused itself uses submit + wait when it is handed page-locked arrays. */
int32_t fpx_phase2_fused_submit(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* round,
                                const int32_t* value_id, const uint64_t* target_mask, uint8_t* chosen,
                                int32_t* chosen_round, int32_t* chosen_value, int32_t* nack_round,
                                int32_t* ticket);
int32_t fpx_phase2_fused_wait(fpx_ctx* ctx, int32_t ticket);
int32_t fpx_phase2_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                             const int32_t* d_value_id, const uint64_t* d_target_mask,
                             uint8_t* d_chosen, int32_t* d_chosen_round, int32_t* d_chosen_value,
                             int32_t* d_nack_round);

/* ---- a2/a4 (K4): Mencius noop ranges -----------------------------------------------------------------
 * Needs FPX_BALLOT_ACCEPTOR.  Rounds must be < 2^30 - 1 everywhere (one key bit marks the per-slot shadow of
 * a length-1 range).  A leader with nothing to propose skips a stretch of its slots with ONE message per
 * stretch; with hundreds of leader groups a tick carries hundreds of them, so every entry point takes n
 * ranges (slot_start[i], slot_end[i], round[i]), processed as if delivered in array order.  Bitmaps are
 * num_groups x 4 words PER RANGE (bit = acceptor index within its acceptor group), so a batch's are
 * n x num_groups x 4.
 *
 * mencius.Acceptor.handlePhase2aNoopRange (mencius/Acceptor.scala:237-291) delivered to the acceptors of
 * EVERY acceptor group of the leader group that owns slot_start (the proxy leader relays a range to each
 * group, mencius/ProxyLeader.scala:276-291), selected by target_masks (NULL = all).  An acceptor with
 * round > `round` Nacks; otherwise round := `round` and every slot of [slot_start, slot_end) owned by its
 * acceptor group (slot = slot_start + k * num_leader_groups with (slot / num_leader_groups) % num_groups ==
 * its group) votes (round, Noop).  Outputs (may be NULL): vote_bits / nack_bits, nack_round[i] = largest round
 * carried by a Nack for range i or -1. */
int32_t fpx_acceptor_phase2a_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start,
                                         const int32_t* slot_end, const int32_t* round,
                                         const uint64_t* target_masks, uint64_t* vote_bits,
                                         uint64_t* nack_bits, int32_t* nack_round);
/* mencius.ProxyLeader.handlePhase2aNoopRange bookkeeping (mencius/ProxyLeader.scala:255-303): opens
 * PendingPhase2aNoopRange for (slot_start, slot_end, round); a known key -- also an earlier message of the
 * same batch -- is ignored (is_new = 0).  The tallies live in a hash table of the context (capacity: a few
 * hundred ranges in flight per leader group; FPX_ECAPACITY beyond it); fpx_proxy_forget reclaims those of
 * a slot window, Pending and Done alike. */
int32_t fpx_proxy_open_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                                   const int32_t* round, uint8_t* is_new);
/* mencius.ProxyLeader.handlePhase2bNoopRange (mencius/ProxyLeader.scala:355-411).  Unknown key ->
 * FPX_EFATAL_UNKNOWN_SLOTROUND; Done or a single-slot tally under the same key -> ignored; ChosenNoopRange
 * (newly_chosen = 1) once every acceptor group has f+1 votes. */
int32_t fpx_proxy_phase2b_noop_ranges(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                                      const int32_t* round, const uint64_t* vote_bits, uint8_t* newly_chosen);
/* Both tallies of a Mencius proxy leader for PER-ACCEPTOR messages, as reference Mencius acceptors send them
 * (mencius/ProxyLeader.scala:305-411): message i of the burst, in delivery order, is a Phase2b(group_index[i],
 * acceptor_index[i], slot[i], round[i]) (kind[i] == FPX_WIRE_PHASE2B, handlePhase2b :305-353) or a
 * Phase2bNoopRange(group_index[i], acceptor_index[i], slot[i] = slot_start, slot_end[i], round[i]) (kind[i] ==
 * FPX_WIRE_PHASE2B_NOOP_RANGE, handlePhase2bNoopRange :355-411) -- the outputs of
 * fpx_wire_mencius_decode_proxy_leader_inbound.  kind == NULL: every message is a Phase2b; a message of any other kind is
 * skipped.  slot_end may be NULL when the burst has no range message.  group_index (NULL = 0) is the range message's
 * acceptor group; a Phase2b's is ignored (its group follows from the slot, :231-235).  The bit of a message is
 * acceptor_index for both kinds.  NO run contract applies: any number of messages per key in any order, several rounds of
 * one key and duplicates are allowed.
 * Contract: the tally state afterwards -- the Phase2b tallies and the range table alike -- equals what this gives: the
 * burst's Phase2b's folded into one row per (slot, round) and handed to fpx_proxy_phase2b, and the burst's range messages
 * folded into one num_groups x 4 row per distinct (slot_start, slot_end, round) in order of first appearance and handed to
 * fpx_proxy_phase2b_noop_ranges.  Each row's outcome is reported at the row's FIRST member message: newly_chosen = 1,
 * chosen_round = round, chosen_value = the value given to fpx_proxy_open, or -1 for a ChosenNoopRange(slot, slot_end)
 * (:395-407); every other message reports newly_chosen = 0, chosen_round = chosen_value = -1.  What
 * fpx_proxy_phase2b_noop_ranges ignores is ignored here: a Done range (:370-376) and a length-1 key held by a single-slot
 * tally (:377-385).  A message whose bit lies outside the member set [0, replicas_total) contributes nothing: it is not
 * looked up, never reports an unknown key and never is its row's first message.  The fold runs on the device
 * (csrc/fpx_mencius_msgs.hpp: claim / gather / tally, one launch each for both kinds; a claim word per range-table entry,
 * allocated by the first call) with integer atomics only: results are reproducible.  Needs FPX_BALLOT_ACCEPTOR and
 * num_leader_groups >= 1, as the range entry points do (FPX_EINVAL otherwise).
 * Errors: FPX_EINVAL with NOTHING applied for acceptor_index outside 0..255, a range message's group_index outside
 * [0, num_groups), a slot outside the window, slot_end < slot or slot_end > num_slots (a range message without a slot_end
 * array included), a round outside 0 .. 2^30 - 2; FPX_EFATAL_UNKNOWN_SLOTROUND per message for a key that was never
 * opened (:309-316, :361-368): that message is dropped, the others are applied.  fpx_error_detail names the LOWEST offending
 * index across both kinds.  n == 0 is FPX_OK.  The host form is synchronous and goes through the staging driver as a
 * single run; the _dev form takes device pointers and enqueues on the context's stream. */
int32_t fpx_mencius_proxy_phase2b_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                       const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                       const int32_t* round, uint8_t* newly_chosen, int32_t* chosen_round,
                                       int32_t* chosen_value);
int32_t fpx_mencius_proxy_phase2b_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                           const int32_t* d_acceptor_index, const int32_t* d_slot,
                                           const int32_t* d_slot_end, const int32_t* d_round, uint8_t* d_newly_chosen,
                                           int32_t* d_chosen_round, int32_t* d_chosen_value);
/* One tick of a Mencius proxy leader among remote acceptors: fpx_mencius_proxy_phase2b_msgs on the six decoded arrays
 * (pageable or page-locked host memory), then the newly chosen records compacted on the device in message order: record k
 * is (out_kind, out_slot = slot or slot_start, out_slot_end = slot_end or -1 for a Chosen, out_round, out_value_id = the
 * value id or -1 for a ChosenNoopRange) -- what the proxy leader sends to every replica as Chosen / ChosenNoopRange
 * (:335-351, :395-407).  *out_count = the number of records.  out_cap (records) too small is FPX_ECAPACITY: the tick WAS
 * applied, *out_count is the count needed and the first out_cap records are written; an unknown-key status outranks it.
 * Every other error is fpx_mencius_proxy_phase2b_msgs': a refused tick applies nothing.  n == 0 is FPX_OK. */
int32_t fpx_mencius_phase2b_tick(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                 const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                 const int32_t* round, int32_t* out_kind, int32_t* out_slot, int32_t* out_slot_end,
                                 int32_t* out_round, int32_t* out_value_id, int32_t out_cap, int32_t* out_count);
/* The fused step for ranges = open + acceptors + tally (the K3 of noop ranges): a range that is already
 * known is neither forwarded nor tallied again.  Outputs may be NULL.  The _dev form takes device pointers,
 * enqueues on the context's stream and needs one round per leader group within the batch (the run contract;
 * FPX_EORDER otherwise, nothing applied); the host form cuts any batch into such runs itself. */
int32_t fpx_noop_ranges_fused(fpx_ctx* ctx, int32_t n, const int32_t* slot_start, const int32_t* slot_end,
                              const int32_t* round, const uint64_t* target_masks, uint64_t* vote_bits,
                              uint64_t* nack_bits, int32_t* nack_round, uint8_t* is_new, uint8_t* chosen);
int32_t fpx_noop_ranges_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot_start,
                                  const int32_t* d_slot_end, const int32_t* d_round,
                                  const uint64_t* d_target_masks, uint64_t* d_vote_bits, uint64_t* d_nack_bits,
                                  int32_t* d_nack_round, uint8_t* d_is_new, uint8_t* d_chosen);
/* One step of a Mencius proxy leader: the Phase2as of the leader groups that have commands AND the Phase2aNoopRanges
 * of the leader groups that skip their slots (mencius/ProxyLeader.scala:231-234 slot -> leader group; :216-303 the two
 * handlers) = fpx_phase2_fused_dev(the first ten arguments) followed by fpx_noop_ranges_fused_dev(the next ten), with
 * exactly their outputs and errors.  independent != 0: the caller states that no leader group has both a command and a
 * range in this step (a leader either proposes in its slots or skips them).  Then the two halves touch disjoint rows,
 * tallies and acceptors, no order between them is observable, and under FPX_F_TRUSTED the step is TWO launches instead
 * of four where its shape allows (groups of at most 32 acceptors on leader-group-major rows, commands delivered to every
 * acceptor -- d_target_mask NULL --, more than 512 commands, a range chain that fits the vote kernel's LDS): the vote
 * kernel with the ranges' chain of dependent steps as its first workgroup, then the ranges' fill with the vote kernel's
 * fold of maxima as further rows of its grid (profiles/r05_cfg5.md); other shapes run the halves side by side, the
 * ranges on a second stream of the context between a fork and a join event.  A context that validates its batches
 * checks the statement first: a leader group with both makes the step FPX_EORDER with nothing applied (call again with
 * independent = 0), and the halves run one after the other.  FPX_BAND_SERIAL=1 in the environment keeps the two-launch
 * form off.  HAZARD: under FPX_F_TRUSTED the statement is NOT checked -- a leader group with both a command and a range
 * in an `independent` step makes the range chain's store of an acceptor's round race with the vote kernel's fold of
 * maxima, and the state is silently wrong.  FPX_DEBUG_CHECKS=1 in the environment checks the statement on trusted contexts too
 * (FPX_EORDER, nothing applied; the halves then run one after the other). */
int32_t fpx_mencius_band_fused_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                                   const int32_t* d_value_id, const uint64_t* d_target_mask, uint8_t* d_chosen,
                                   int32_t* d_chosen_round, int32_t* d_chosen_value, int32_t* d_nack_round,
                                   int32_t n_ranges, const int32_t* d_slot_start, const int32_t* d_slot_end,
                                   const int32_t* d_range_round, const uint64_t* d_range_target_masks,
                                   uint64_t* d_range_vote_bits, uint64_t* d_range_nack_bits,
                                   int32_t* d_range_nack_round, uint8_t* d_range_is_new, uint8_t* d_range_chosen,
                                   int32_t independent);
/* diagnostic: the fused steps since fpx_create whose launch carried the fold of the step before in its own grid.  Every K1 /
 * K3 launch is followed by a fold of the maxima its workgroups left (Acceptor.round / maxVotedSlot, multipaxos/Acceptor.scala:
 * 204-209, as scalars per acceptor); with a ballot per cell (FPX_BALLOT_PER_SLOT) no vote kernel reads those scalars, so the
 * fold of one fpx_phase2_fused_dev call waits for the next one and rides in its launch (or is launched by whatever entry
 * point other than a Phase1a touches the context first: the deferral is not observable through this ABI).  FPX_NO_DEFER_FINALIZE=1 in the
 * environment launches every fold at once, as rounds 1 - 5 did. */
int64_t fpx_deferred_folds(fpx_ctx* ctx);
/* diagnostic: the steps of fpx_mencius_band_fused_dev that ran in the two-launch form since fpx_create */
int64_t fpx_band_merged_steps(fpx_ctx* ctx);
/* diagnostic: a census of the vote launches (K1 / K3, the kernel k_phase2 and its forms) since fpx_create -- plain host
 * counters, bumped where the host chooses a launch; nothing runs on the device and reading them launches nothing (not even a
 * pending fold).  fpx_reset does NOT clear them (nor fpx_deferred_folds / fpx_band_merged_steps): they count the life of
 * the context.  Writes min(cap, FPX_CENSUS_WORDS) int64 words to out and FPX_CENSUS_WORDS to *n (either may be NULL).
 *
 * Words [0, FPX_CENSUS_CELLS * FPX_CENSUS_FORMS): counts[cell * FPX_CENSUS_FORMS + form], cell = FPX_CENSUS_CELL(...):
 *   G       lanes per slot (1, 2, 4, ... 64: the smallest power of two with 4 G >= num_replicas)
 *   mode    0 dense delivery, 1 target masks, 2 target masks + FPX_F_SCATTERED_TARGETS, 3 the packed walk (G = 64)
 *   ps      0 a round per acceptor (FPX_BALLOT_ACCEPTOR), 1 a ballot per cell, 2 a ballot per cell with lazy Phase1a
 *           promises outstanding
 *   fused   0 K1 (fpx_acceptor_phase2a*), 1 K3 (fpx_phase2_fused*, fpx_mencius_band_fused_dev)
 * Every vote launch counts once under one of the first four forms, in its own cell:
 *   FPX_CENSUS_SOLO   one workgroup that applies its maxima itself (no fold follows)
 *   FPX_CENSUS_GRID   several workgroups, k_phase2: a fold of their per-workgroup maxima rows follows (below)
 *   FPX_CENSUS_FIN    several workgroups, k_phase2_fin: the grid also carries the fold of the launch before
 *   FPX_CENSUS_BAND   k_phase2_band: a Mencius band's vote kernel with the range chain as its first workgroup
 *                     (its fold rides in the fill behind it)
 * and the fold of every FPX_CENSUS_GRID / FPX_CENSUS_FIN launch counts once under one of the other four, in the cell of
 * the launch whose maxima it folds:
 *   FPX_CENSUS_FOLD_NOW      launched by itself (k_finalize) right behind its vote launch
 *   FPX_CENSUS_FOLD_BEHIND   left pending, then launched by itself right behind the NEXT vote launch (the widths
 *                            without k_phase2_fin: the two launches use the two halves of the maxima rows)
 *   FPX_CENSUS_FOLD_CARRIED  left pending, then carried in the next vote launch's grid (FPX_CENSUS_FIN there)
 *   FPX_CENSUS_FOLD_FLUSHED  left pending, then launched by itself by an entry point or ahead of a solo launch
 *   (a fold still pending when the census is read is not counted yet)
 * Then three words: FPX_CENSUS_CAPPED  the vote launches whose grid was capped below what the batch needed (every
 * wavefront walks several chunks); FPX_CENSUS_SC_LDS  those that had LDS for the column quads of a slot-ordered batch
 * (leader-group-major rows and every array 16-byte aligned); FPX_CENSUS_TH_LDS  those that staged the acceptors'
 * rounds of every group per workgroup. */
enum {
  FPX_CENSUS_SOLO = 0,
  FPX_CENSUS_GRID = 1,
  FPX_CENSUS_FIN = 2,
  FPX_CENSUS_BAND = 3,
  FPX_CENSUS_FOLD_NOW = 4,
  FPX_CENSUS_FOLD_BEHIND = 5,
  FPX_CENSUS_FOLD_CARRIED = 6,
  FPX_CENSUS_FOLD_FLUSHED = 7,
  FPX_CENSUS_FORMS = 8,
  FPX_CENSUS_CELLS = 7 * 4 * 3 * 2,
  FPX_CENSUS_CAPPED = FPX_CENSUS_CELLS * FPX_CENSUS_FORMS,
  FPX_CENSUS_SC_LDS = FPX_CENSUS_CAPPED + 1,
  FPX_CENSUS_TH_LDS = FPX_CENSUS_CAPPED + 2,
  FPX_CENSUS_WORDS = FPX_CENSUS_CAPPED + 3
};
/* the census cell of (G, mode, ps, fused) as above: G_log2 = log2(G) */
#define FPX_CENSUS_CELL(G_log2, mode, ps, fused) ((((G_log2) * 4 + (mode)) * 3 + (ps)) * 2 + (fused))
int32_t fpx_vote_launch_census(fpx_ctx* ctx, int32_t cap, int64_t* out, int32_t* n);
/* diagnostic: a census of the noop-range launches (K4, fpx_ranges.hpp) since fpx_create -- plain host counters like those
 * of fpx_vote_launch_census, bumped where the host chooses a launch, once per device run (the host entry points cut a
 * batch into runs of one round per leader group); reading them launches nothing and fpx_reset treats them as it treats the
 * vote census (they count the life of the context).  Writes min(cap, FPX_RANGE_CENSUS_WORDS) int64 words to out and
 * FPX_RANGE_CENSUS_WORDS to *n (either may be NULL).  A fused run (fpx_noop_ranges_fused*, the ranges of
 * fpx_mencius_band_fused_dev) counts once under one of
 *   FPX_RANGE_CENSUS_CHAIN   k_ranges_chain: one workgroup walks open -> resolve -> acceptors -> tally
 *   FPX_RANGE_CENSUS_STEPS   the same steps as launches of their own (k_ranges_open, _resolve, _acceptors, _tally): more
 *                            than 2048 ranges, more LDS than the chain may take, or more than 8192 acceptor threads
 *   FPX_RANGE_CENSUS_BAND    the chain as the first workgroup of a band's vote kernel (k_phase2_band), its fill in
 *                            k_ranges_fill_lg_fin (counted under no fill word)
 * the unfused entry points once under FPX_RANGE_CENSUS_OPEN_ONLY (fpx_proxy_open_noop_range*),
 * FPX_RANGE_CENSUS_ACCEPTORS_ONLY (fpx_acceptor_phase2a_noop_range*) or FPX_RANGE_CENSUS_TALLY_ONLY
 * (fpx_proxy_phase2b_noop_range*), and every run with an acceptor step outside a band once under its fill:
 *   FPX_RANGE_CENSUS_FILL_LG     k_ranges_fill_lg (leader-group-major rows)
 *   FPX_RANGE_CENSUS_FILL_SWEEP  k_ranges_fill_rows (slot-ordered rows, at most 1024 ranges and 2048 leader groups)
 *   FPX_RANGE_CENSUS_FILL_RANGE  k_ranges_fill (slot-ordered rows otherwise)
 * FPX_RANGE_CENSUS_REHASH counts the moves of the range tallies to their other buffer (fpx_proxy_forget,
 * fpx_recycle_slots with a window of at least one slot). */
enum {
  FPX_RANGE_CENSUS_CHAIN = 0,
  FPX_RANGE_CENSUS_STEPS = 1,
  FPX_RANGE_CENSUS_BAND = 2,
  FPX_RANGE_CENSUS_FILL_LG = 3,
  FPX_RANGE_CENSUS_FILL_SWEEP = 4,
  FPX_RANGE_CENSUS_FILL_RANGE = 5,
  FPX_RANGE_CENSUS_TALLY_ONLY = 6,
  FPX_RANGE_CENSUS_OPEN_ONLY = 7,
  FPX_RANGE_CENSUS_ACCEPTORS_ONLY = 8,
  FPX_RANGE_CENSUS_REHASH = 9,
  FPX_RANGE_CENSUS_WORDS = 10
};
int32_t fpx_range_launch_census(fpx_ctx* ctx, int64_t* out, int32_t cap, int32_t* n);
/* batches of one (bitmaps num_groups x 4 words) */
int32_t fpx_acceptor_phase2a_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end,
                                        int32_t round, const uint64_t* target_masks,
                                        uint64_t* vote_bits, uint64_t* nack_bits, int32_t* nack_round);
int32_t fpx_proxy_open_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round,
                                  uint8_t* is_new);
int32_t fpx_proxy_phase2b_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round,
                                     const uint64_t* vote_bits, uint8_t* newly_chosen);
/* readback (parity): state 0 = unknown key, 1 = Pending, 2 = Done; vote_bits num_groups x 4 words (zero
 * unless Pending) */
int32_t fpx_read_range_tally(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, int32_t* state,
                             uint64_t* vote_bits);
/* readback (parity) of where that tally lives in the context's open-addressing table: capacity = the table's buckets (a
 * power of two; at most capacity / 2 entries are live), home_bucket = the bucket the key's hash selects, computed on the
 * device, bucket = the one the entry was found in by linear probing from there (wrapping from the last bucket to bucket
 * 0), or -1 for an unknown key.  Any output may be NULL. */
int32_t fpx_read_range_position(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end, int32_t round, int32_t* capacity,
                                int32_t* home_bucket, int32_t* bucket);

/* ---- a9 (K5): EPaxos pre-accept fast path -------------------------------------------------------------
 * One tick of FRESH instances through the pre-accept phase of n = 2f+1 EPaxos replicas with the
 * key-value store's top-one conflict index (epaxos/Replica.scala:569-600, 633-729, 1159-1419;
 * statemachine/KeyValueStore.scala:225-302; util/TopOne.scala; Util.scala:19-21).
 *
 * Message i: instance (leader[i], number[i]) with a single-key command on key[i] (is_set[i] = 1:
 * SetRequest, 0: GetRequest); the leader sends PreAccept to the n-2 other replicas in resp_mask[i]
 * (thrifty fast quorum, Replica.scala:705-706).  rank is n x m: rank[r * m + i] = the position of
 * message i in replica r's processing order (a permutation of 0..m-1 per replica; only replicas that
 * take part in message i -- its leader and resp_mask[i] -- matter; a rank row that is not a permutation
 * is FPX_EINVAL and nothing is applied; values outside 0..m-1 are always caught, and a row whose values are in
 * range but repeat is told from a permutation by comparing two independent 64-bit additive fingerprints of its
 * multiset of values with those of 0..m-1 -- no scatter / gather of the row is needed for it).  Every participating replica
 * computes the command's conflicts against ITS conflict index in ITS order (getTopOneConflicts), the
 * leader's become the PreAccept's dependencies, the others answer PreAcceptOk with the union; the
 * leader takes the fast path iff the n-2 answers are identical (popularItems(..., n-2)), otherwise
 * the slow path proposes the union of all answers (preAcceptingSlowPath, :796-813).  After the tick
 * the commits reach every replica's conflict index (commit -> updateConflictIndex, :815-828).
 * seen_mask (NULL = resp_mask, the thrifty deployment): the OTHER replicas that receive and process the
 * PreAccept at all.  With the reference's default ThriftySystem.NotThrifty (Replica.scala:83, 556-562) that is
 * every other replica (n-1 of them): all of them compute conflicts and update their index in their order,
 * and the leader decides on the first n-2 answers to arrive (fastQuorumSize responses including its own,
 * :1376) -- resp_mask, a subset of seen_mask.
 * Outputs (may be NULL): fast[i]; deps = the committed (fast) or Accept-phase (slow) dependencies and
 * leader_deps = the PreAccept's, as InstancePrefixSets (epaxos/InstancePrefixSet.scala): deps[i * n + l] is
 * the IntPrefixSet watermark of leader l's column (every instance of l below it is a dependency).  The
 * reference removes the instance itself from its dependencies (dependencies.subtractOne(instance),
 * Replica.scala:582; compact/IntPrefixSet.scala:388-398), which only ever changes the column of the
 * instance's OWN leader: when a replica already holds a higher-numbered conflicting instance of that leader
 * (it processed (L, 5) before (L, 4)), that column's watermark drops to number[i] and the ids above it become
 * the set's explicit `values` -- always the run number[i] + 1 .. end - 1, reported as
 * own_values_end[i * 2 + 0] (deps) and own_values_end[i * 2 + 1] (leader_deps); 0 = no explicit values (the
 * case on every FIFO channel).  Sequence numbers are the constant 0 the reference uses with top-k
 * dependencies (:575-578). */
typedef struct fpx_epx fpx_epx;
typedef struct {
  int32_t num_replicas; /* n: 3, 5 or 7 */
  int32_t num_keys;
  int32_t device;
  uint32_t flags;
  int32_t num_instances; /* > 0: every replica keeps its command log (Replica.cmdLog) for the instances
                            (leader, number < num_instances): fpx_epx_preaccept records and checks it,
                            fpx_epx_prepare / fpx_epx_accept run on it.  0: no command log (pre-accept only) */
} fpx_epx_config;
int32_t fpx_epx_create(const fpx_epx_config* cfg, fpx_epx** out);
int32_t fpx_epx_destroy(fpx_epx* epx);
/* n, num_keys, num_instances of the context (any pointer may be NULL) */
int32_t fpx_epx_info(fpx_epx* epx, int32_t* num_replicas, int32_t* num_keys, int32_t* num_instances);
/* the exact-fit limits of the pre-accept tick for the context's n, so that tests and tools read them and do not restate
 * them.  Writes min(cap, FPX_EPX_LIMIT_WORDS) int32 words to out and FPX_EPX_LIMIT_WORDS to *n (either may be NULL):
 *   FPX_EPX_LIMIT_KP_TC       commands of one key the second form (partition by key, k_epx_key2) holds on chip
 *   FPX_EPX_LIMIT_KEY_TC      commands of one key the first form's per-key kernel (k_epx_key) holds on chip
 *   FPX_EPX_LIMIT_NBK         rank buckets of the second form's bucket sort
 *   FPX_EPX_LIMIT_KP_MAX_OCC  words of one replica in the fullest bucket that sort accepts
 *   FPX_EPX_LIMIT_KP_MAXB     keys the second form takes
 *   FPX_EPX_LIMIT_KP_WAVES    wavefronts per replica in k_epx_key2 (a key's slots are split among them in runs of 64) */
enum {
  FPX_EPX_LIMIT_KP_TC = 0,
  FPX_EPX_LIMIT_KEY_TC = 1,
  FPX_EPX_LIMIT_NBK = 2,
  FPX_EPX_LIMIT_KP_MAX_OCC = 3,
  FPX_EPX_LIMIT_KP_MAXB = 4,
  FPX_EPX_LIMIT_KP_WAVES = 5,
  FPX_EPX_LIMIT_WORDS = 6
};
int32_t fpx_epx_limits(fpx_epx* epx, int32_t cap, int32_t* out, int32_t* n);
/* diagnostic: a census of the paths the single-key pre-accept ticks (fpx_epx_preaccept, _dev, _packed_dev; not the _mk
 * entry points) took since fpx_epx_create -- the counters cover the life of the context, like those of
 * fpx_vote_launch_census.  Writes min(cap, FPX_EPX_CENSUS_WORDS) int64 words to out and FPX_EPX_CENSUS_WORDS to *n (either
 * may be NULL); reading waits for the context's stream and copies two small blocks of device words (64 and 40 bytes), it
 * launches nothing.
 * Host words, bumped where the host decides; a tick counts under exactly one of the first seven:
 *   FPX_EPX_CENSUS_KP               taken by the second form (k_kp_hist, k_kp_scatter, k_epx_key2) and not handed over.  It is
 *                                   counted when the partition reports that every key fits: a tick k_epx_key2 then refuses
 *                                   (a bad message, rank rows that are no permutations: FPX_EINVAL, nothing applied)
 *                                   counts here as well, its keys under no sort route
 *   FPX_EPX_CENSUS_KP_HANDED_OVER   partitioned by the second form, which found a key with more commands than its
 *                                   on-chip tables hold: nothing was applied, the first form took the whole tick
 *   sent to the first form by dispatch, without a partition launch -- the first reason that holds, in this order:
 *   FPX_EPX_CENSUS_V1_SWITCHED_OFF  FPX_EPX_V1 in the environment at fpx_epx_create (or no page-locked word to be had)
 *   FPX_EPX_CENSUS_V1_KEYS          num_keys > FPX_EPX_LIMIT_KP_MAXB
 *   FPX_EPX_CENSUS_V1_FULL          m > num_keys * FPX_EPX_LIMIT_KP_TC: some key must overflow
 *   FPX_EPX_CENSUS_V1_LOG_N3        n = 3 with a command log (or a triple_id array)
 *   FPX_EPX_CENSUS_V1_INDEX_BITS    m >= 2^21
 * and beside them
 *   FPX_EPX_CENSUS_NO_KEY_KERNEL    first-form ticks that ran k_epx_scan / k_epx_decide without the per-key kernel k_epx_key
 *   FPX_EPX_CENSUS_SCALAR_LOADS     partition launches (applied or handed over) that read the tick element by element:
 *                                   an input array off a 16-byte boundary, or m % 4 != 0
 * Device words, read when the census is read.  Non-empty keys of the second-form ticks that were applied, by the route that put their
 * sort words in rank order.  k_epx_key2 sorts a key's n replicas side by side and ONE replica's overfull bucket sends all
 * of them to the next route, so a key counts once, under the route of its worst replica:
 *   FPX_EPX_CENSUS_SORT_BUCKET1     bucket sort over the tick's ranks [0, m)
 *   FPX_EPX_CENSUS_SORT_BUCKET2     bucket sort over the key's own rank range, after the first attempt met a bucket of
 *                                   more than FPX_EPX_LIMIT_KP_MAX_OCC words
 *   FPX_EPX_CENSUS_SORT_RADIX1 .. 3 LSD radix sort of 1, 2, 3 passes of 7 bits (ceil(bits(m) / 7)), after both attempts did
 *   FPX_EPX_CENSUS_LONG_WAY         keys the first form's k_epx_key left to k_epx_scan / k_epx_decide (more commands than
 *                                   FPX_EPX_LIMIT_KEY_TC), summed over the ticks */
enum {
  FPX_EPX_CENSUS_KP = 0,
  FPX_EPX_CENSUS_KP_HANDED_OVER = 1,
  FPX_EPX_CENSUS_V1_SWITCHED_OFF = 2,
  FPX_EPX_CENSUS_V1_KEYS = 3,
  FPX_EPX_CENSUS_V1_FULL = 4,
  FPX_EPX_CENSUS_V1_LOG_N3 = 5,
  FPX_EPX_CENSUS_V1_INDEX_BITS = 6,
  FPX_EPX_CENSUS_NO_KEY_KERNEL = 7,
  FPX_EPX_CENSUS_SCALAR_LOADS = 8,
  FPX_EPX_CENSUS_SORT_BUCKET1 = 9,
  FPX_EPX_CENSUS_SORT_BUCKET2 = 10,
  FPX_EPX_CENSUS_SORT_RADIX1 = 11,
  FPX_EPX_CENSUS_SORT_RADIX2 = 12,
  FPX_EPX_CENSUS_SORT_RADIX3 = 13,
  FPX_EPX_CENSUS_LONG_WAY = 14,
  FPX_EPX_CENSUS_WORDS = 15
};
int32_t fpx_epx_tick_census(fpx_epx* epx, int32_t cap, int64_t* out, int32_t* n);
int32_t fpx_epx_set_stream(fpx_epx* epx, void* hip_stream);
int32_t fpx_epx_preaccept(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                          const int32_t* key, const uint8_t* is_set, const uint8_t* resp_mask,
                          const uint8_t* seen_mask, const int32_t* rank, const int32_t* triple_id,
                          uint8_t* fast, int32_t* deps, int32_t* leader_deps, int32_t* own_values_end);
/* device-resident inputs / outputs; the work is enqueued on the context's stream and fpx_epx_sync returns the sticky
 * status.  One host wait is inside: for ticks of at most 2048 keys the library partitions the tick by key and runs
 * one kernel per key group on chip, which needs every key's commands to fit the on-chip tables (1152 per key at
 * n = 5); whether they do is known once the tick's key histogram is -- a few microseconds of device work after the
 * stream reaches this call -- and is read from a page-locked word while the next kernels (already enqueued) run.  The
 * call therefore returns when the stream has reached the tick's first two small kernels, not before; a tick with a
 * hotter key is then enqueued again in the general form (radix sort of all (key, message) pairs).  Not capturable
 * into a HIP graph.  FPX_EPX_V1 in the environment at fpx_epx_create selects the general form always.
 * Any alignment of the input arrays is accepted; arrays that all start at 16-byte boundaries, with m % 4 == 0, are read
 * with 16-byte loads (~1 % of a 2^20-command tick). */
int32_t fpx_epx_preaccept_dev(fpx_epx* epx, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                              const int32_t* d_key, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                              const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id,
                              uint8_t* d_fast, int32_t* d_deps, int32_t* d_leader_deps,
                              int32_t* d_own_values_end);
/* The same with ONE packed line per command instead of the four output arrays (what the kernel that decides a key
 * writes most cheaply: a command's outputs are contiguous and sector-aligned, where the four arrays take four
 * partial sectors at every message index).  d_packed: m x fpx_epx_packed_stride(n) ints; line i =
 *   [0, n) deps   [n, 2n) leader_deps   [2n] own_values_end (deps)   [2n + 1] own_values_end (leader_deps)
 *   [2n + 2] fast (0 / 1)   the rest 0            (stride = 12 / 16 / 20 ints for n = 3 / 5 / 7) */
int32_t fpx_epx_packed_stride(int32_t num_replicas);
int32_t fpx_epx_preaccept_packed_dev(fpx_epx* epx, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                     const int32_t* d_key, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                                     const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id,
                                     int32_t* d_packed);
int32_t fpx_epx_sync(fpx_epx* epx);
/* Dependency-graph execution of one tick's commits ON THE DEVICE (the general, host-side graph is
 * include/fpx_depgraph.h): what Replica.execute does with the committed triples (epaxos/Replica.scala:859-917,
 * depgraph/TarjanDependencyGraph.scala:225-276) -- strongly connected components of the committed instances, components
 * in reverse topological order, inside a component by (leader, id) (sequence numbers are 0 with top-k dependencies).
 * Message i = instance (leader[i], number[i]) with the dependencies of line i of d_packed (fpx_epx_preaccept_packed_dev's
 * output: deps watermarks + the explicit ids of the own column); d_committed (may be NULL = all) 0 = not committed yet:
 * it and whatever reaches it wait.  The columns must be DENSE: leader l's instances first[l] .. first[l] + count[l] - 1
 * each exactly once (sum of count = m), everything below first[l] executed earlier (FPX_EINVAL otherwise).
 * Ids: 0 <= first[l] and first[l] + count[l] <= 2^31 - 2 for every column (FPX_EINVAL otherwise, nothing is run), so that
 * every instance id is at most 2^31 - 3 and a watermark can still name an instance beyond the column's end; watermarks are
 * any int32 >= 0 (negative: FPX_EINVAL), one above first[l] + count[l] makes the instance wait.  m < 2^21.  (With int32
 * first and count and m < 2^21, the one end this refuses that int32 ids could still hold is 2^31 - 1: there no watermark
 * could lie beyond the column; larger sums do not fit an id at all.)
 * Outputs: d_order[p] = the message executed p-th, d_component[p] = its component's number (consecutive from 0; equal
 * numbers = one strongly connected component), for p < *num_executed; *num_components.  Where the reference leaves the
 * order open (components that do not depend on each other) this path takes its own; the SET of components and the
 * validity of the order equal fpx_depgraph's.  *needs_host_path != 0: the members of a strongly connected component could
 * not be made neighbours of the order -- two DIFFERENT closures of vertices on cycles have the same closure sum AND the same
 * 22-bit closure hash, so their members may interleave (detected where component starts are found; components of any size
 * are handled on the device, this is a hash collision, probability ~2^-22 per pair of such closures), or a closure sum of
 * 2^29 and more (not reachable with m < 2^21) -- the outputs are not valid, run the tick through fpx_depgraph_commit_epx.
 * Device pointers, the context's stream; ONE host wait on a page-locked word at the end (round 4: one per closure round),
 * so the call returns when the order is on the device: not capturable into a HIP graph.  n <= 5 with columns of fewer
 * than 2^21 - 2 instances runs on 16-byte rows (csrc/fpx_depgraph_pk.hpp), everything else on 32-byte rows;
 * FPX_DG_WIDE=1 in the environment forces the latter (the results do not depend on it); FPX_DG_HASH_BITS=b (2 .. 22) shortens
 * the closure hash -- a test hook that makes the collisions needs_host_path reports happen (tests/test_depgraph_dev.py). */
int32_t fpx_epx_execute_dev(fpx_epx* epx, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                            const int32_t* d_packed, const uint8_t* d_committed, const int32_t* first,
                            const int32_t* count, int32_t* d_order, int32_t* d_component, int64_t* num_executed,
                            int64_t* num_components, int32_t* needs_host_path);
/* The same on HOST arrays (what a JNI caller holds: frankenpaxos_amd/jni/EPaxosNative.scala, `deviceExecution`): message i
 * = instance (leader[i], number[i]) committed with the watermarks deps[i * n .. i * n + n) and, if deps_values_end is given
 * and deps_values_end[i] > 0, the explicit ids number[i] + 1 .. deps_values_end[i] - 1 of its own column
 * (dependencies.subtractOne, Replica.scala:582; then deps[i * n + leader[i]] must equal number[i]); committed (may be NULL =
 * all) as above.  order / component: m entries each, filled for p < *num_executed.  Builds the packed lines, uploads,
 * runs fpx_epx_execute_dev, downloads; synchronous. */
int32_t fpx_epx_execute(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* deps,
                        const int32_t* deps_values_end, const uint8_t* committed, const int32_t* first,
                        const int32_t* count, int32_t* order, int32_t* component, int64_t* num_executed,
                        int64_t* num_components, int32_t* needs_host_path);

/* ---- EPaxos beyond fresh instances: the per-instance Paxos on the command log (num_instances > 0) --------------
 * Ballots are (ordering, replicaIndex), compared lexicographically (epaxos/BallotHelpers.scala:11-21); where one
 * int32 carries a ballot it is ordering * 8 + replicaIndex, the null ballot (-1, -1) (Replica.scala:256) is -1.
 * Command-log entry kinds: 0 none, 1 NoCommandEntry, 2 PreAcceptedEntry, 3 AcceptedEntry, 4 CommittedEntry
 * (Replica.scala:303-330).  A CommandTriple is the caller's int32 triple_id (the command; pre-accept: the optional
 * triple_id argument) plus its dependencies, which the command log keeps with every entry a pre-accept wrote (what
 * THAT replica answered, :1259-1271; the agreed dependencies after a fast-path commit): n watermarks + the end of
 * the own-leader column's explicit values (fpx_epx_read_cmdlog_deps).  An Accept names its triple by id alone:
 * the entries it writes have dependency column 0 = -1 ("look the triple up by its id").
 * fpx_epx_preaccept with a command log: every participating replica must not know the instance yet (the
 * `cmdLog.get == None` branch of handlePreAccept, Replica.scala:1169-1172; anything else is FPX_EINVAL, nothing
 * applied); it records PreAcceptedEntry(Ballot(0, leader), Ballot(0, leader), triple) at the participants, and a
 * fast-path commit turns the entry into CommittedEntry at every replica.
 *
 * The three calls below deliver message i, in array order, to the replicas in target_mask[i] (bit r); the instances
 * (leader[i], number[i]) of one call must be pairwise distinct (FPX_EINVAL otherwise, nothing applied).  Replies
 * per message (host pointers, may be NULL): ok_bits / nack_bits / commit_bits (the replica answered with the Commit
 * it already holds), nack_ballot = the largest `largestBallot` carried by a Nack (Nack(instance, largestBallot),
 * Replica.scala:1424, 1652), -1 if none.
 *
 * fpx_epx_prepare: Replica.handlePrepare (Replica.scala:1632-1757) -- phase 1 of an instance's recovery.  reply_*
 *   are m x n: the PrepareOk of replica r = (status: 0 NotSeen / 2 PreAccepted / 3 Accepted, voteBallot, triple id);
 *   -1 where r sent no PrepareOk.
 * fpx_epx_accept: the Accept phase of message i proposed by replica ballot_replica[i] in ballot
 *   (ballot_ordering[i], ballot_replica[i]): transitionToAcceptPhase at the proposer (:732-792; target_mask must
 *   not contain it), handleAccept at the targets (:1421-1511), handleAcceptOk (:1513-1565): with f + 1 responses,
 *   the proposer's own included, the instance is committed -- CommittedEntry at every replica (commit :815-860 and
 *   Commit to the others).  A proposer that holds a CommittedEntry, or an entry with a larger ballot, would have
 *   died in logger.fatal / logger.check: FPX_EFATAL_PROTOCOL, that message is skipped.
 *   key[i] / is_set[i] = the triple's command (key -1 = Noop): wherever the reference stores the triple it also calls
 *   updateConflictIndex(instance, commandOrNoop) (:602-614) -- at the proposer (:763), at every replica that takes
 *   the Accept in (:1503) and, on commit, at every replica (:828) -- so a replica that first hears of an instance
 *   through an Accept or a Commit reports it as a conflict from then on. */
int32_t fpx_epx_prepare(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                        const int32_t* ballot_ordering, const int32_t* ballot_replica, const uint8_t* target_mask,
                        uint8_t* ok_bits, uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot,
                        int32_t* reply_status, int32_t* reply_vote_ballot, int32_t* reply_triple);
/* K8: Replica.handlePrepareOk (epaxos/Replica.scala:1759-1884) -- the decision of the replica that recovers instance i
 * in ballot (ballot_ordering[i], ballot_replica[i]) once it holds the PrepareOks of the replicas in resp_mask[i]
 * (fpx_epx_prepare's ok_bits) with the contents reply_* (fpx_epx_prepare's outputs, m x n):
 *   action 0 = fewer than f + 1 responses, wait (:1799-1801)
 *   action 1 = transitionToAcceptPhase(instance, ballot, the triple replica `source` reported)     -> fpx_epx_accept
 *   action 2 = transitionToPreAcceptPhase(instance, ballot, the command of `source`'s triple, avoidFastPath = true)
 *   action 3 = transitionToPreAcceptPhase(instance, ballot, Noop, avoidFastPath = true)  -> fpx_epx_handle_preaccept
 * triple[i] = that triple's id (-1 for action 0 / 3); source = the lowest replica index among the eligible responses
 * (the reference takes whichever its hash map yields first; they carry the same command).
 * as_intended = 0 reproduces the reference AS IT EVALUATES: its test for an Accepted response compares the required
 * enum field `status` with an Option (:1810, always false) and its default-ballot filter looks at the ballot of the
 * Prepare that was answered instead of the vote's (:1831, never the default ballot during a recovery), so only
 * actions 0, 2 and 3 can come out.  as_intended = 1 evaluates the two tests the way the surrounding comments describe
 * them (an Accepted response at the highest voteBallot wins; f identical PreAccepted triples voted in
 * Ballot(0, leader), the recovering replica's own excluded, win: Util.popularItems(.., f) with the triples compared as
 * the command log stores them).  Reads the command log, changes nothing.  The PrepareOks' triples are compared through
 * the command-log entries they were answered from (reply_triple names a triple, the entry holds its dependencies): the
 * caller must not let another call touch these instances between fpx_epx_prepare and this one -- a decision taken on
 * entries that moved meanwhile is taken on other data than the PrepareOks carried (the reference's replies carry the
 * triples themselves, Replica.scala:1717-1731). */
int32_t fpx_epx_handle_prepare_oks(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                                   const int32_t* ballot_ordering, const int32_t* ballot_replica,
                                   const uint8_t* resp_mask, const int32_t* reply_status,
                                   const int32_t* reply_vote_ballot, const int32_t* reply_triple, int32_t as_intended,
                                   int32_t* action, int32_t* source, int32_t* triple);
int32_t fpx_epx_accept(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                       const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* triple_id,
                       const int32_t* key, const uint8_t* is_set, const uint8_t* target_mask, uint8_t* ok_bits,
                       uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot, uint8_t* committed);
/* K7: Replica.handlePreAccept in full (epaxos/Replica.scala:1159-1289) -- what fpx_epx_preaccept's tick-at-once form
 * leaves out: PreAccepts for instances a replica already knows (a leader's re-sent PreAccept, a recovering replica
 * pre-accepting again in a higher ballot).  Message i = PreAccept(instance (leader, number), ballot
 * (ballot_ordering, ballot_replica), single-key get / set on key[i] or Noop (key[i] = -1), sequenceNumber 0,
 * dependencies deps_in[i * n ..] = n watermarks + deps_in_values_end[i] (explicit values number + 1 .. end - 1 of
 * the instance's own-leader column, 0 = none; the array may be NULL; a PreAccept that depends on its own instance is
 * FPX_EINVAL)), delivered in array order to the replicas of target_mask[i]; instances pairwise distinct per call.
 * At each replica, cmdLog.get(instance) decides (:1169-1238):
 *   none                                            -> processed
 *   NoCommandEntry(b):       ballot < b             -> Nack(instance, largestBallot)
 *   PreAcceptedEntry(b, vb): ballot < b -> Nack;  ballot == vb -> the PreAcceptOk again, from the stored triple
 *   AcceptedEntry(b, vb):    ballot < b -> Nack;  ballot == vb -> ignored
 *   CommittedEntry(triple)                          -> the Commit back
 *   otherwise processed: largestBallot = max(largestBallot, ballot) (:1251); dependencies = the command's conflicts
 *   in THIS replica's index minus the instance itself (computeSequenceNumberAndDependencies :569-600; none for a
 *   Noop) U deps_in (:1257-1262); PreAcceptedEntry(ballot, ballot, triple) (:1265-1276); updateConflictIndex (:1279,
 *   a Noop leaves the index alone); PreAcceptOk(dependencies).  (The leaderStates / timer bookkeeping of :1243-1254
 *   is leader-side state outside this path.)
 * Replies (host pointers, may be NULL): ok_bits (processed), resend_bits, nack_bits, commit_bits -- the other replicas
 * of target_mask ignored the message; nack_ballot as above; reply_deps (m x n x n) / reply_values_end (m x n) /
 * reply_triple (m x n): the dependencies and triple id of the PreAcceptOk or Commit replica r sent (zeros / 0 / -1
 * where it sent neither). */
int32_t fpx_epx_handle_preaccept(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                                 const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* key,
                                 const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps_in,
                                 const int32_t* deps_in_values_end, const uint8_t* target_mask, uint8_t* ok_bits,
                                 uint8_t* resend_bits, uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot,
                                 int32_t* reply_deps, int32_t* reply_values_end, int32_t* reply_triple);
/* Replica.handleCommit (epaxos/Replica.scala:1567-1575 -> commit, :815-830) at every replica of target_mask: whatever the
 * replica's command log held for the instance is replaced by CommittedEntry(triple) -- a Commit is final, no ballot is
 * compared (:826-827) -- and its conflict index learns the command (:828; key -1 = Noop).  deps: n watermarks per
 * message + deps_values_end (the explicit ids number + 1 .. end - 1 of the own-leader column, 0 = none), or NULL: the
 * triple is known by its id alone, as after an Accept.  Instances of one call that repeat must carry the same triple.
 * Timers, leaderStates and the dependency graph (:822, :831, :859-875) are the caller's.  FPX_EINVAL, nothing applied:
 * an instance outside the command log, a key outside the index, a replica outside target_mask's n bits, negative
 * watermarks, explicit ids that do not lie above the instance. */
int32_t fpx_epx_handle_commit(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                              const int32_t* triple_id, const int32_t* key, const uint8_t* is_set, const int32_t* deps,
                              const int32_t* deps_values_end, const uint8_t* target_mask);
/* ---- multi-key get / set commands: one _mk form per entry point above that takes a command ----------------------
 * The reference's key-value store takes GetRequest / SetRequest with any number of keys (statemachine/KeyValueStore.scala
 * :221-302, typedTopKConflictIndex with k = 1): a command's top-one conflicts are the element-wise max, over its keys, of
 * each key's TopOne (a get merges the sets of its keys, a set their gets and sets), and put records the instance under
 * every key of the command.  The _mk forms take, in place of key[m], a CSR key list:
 *   key_offsets[m + 1]  key_offsets[0] = 0, non-decreasing; command i's keys are keys[key_offsets[i] .. key_offsets[i + 1])
 *   keys[key_offsets[m]]  each in [0, num_keys); is_set[m] per command (the reference's command is a GetRequest or a
 *                         SetRequest, not a mix)
 * A key repeated inside one command counts once (the reference's merge and put are idempotent); the library drops the
 * repeats itself.  A command with NO keys gets the empty set as its conflicts (snapshots, which EPaxos never fills: it
 * never calls putSnapshot) and put adds nothing -- on the device it behaves exactly like a Noop (no dependencies, the
 * index untouched), while it stays a command for the caller's triple.  Offsets that are not monotone, a key out of
 * range or more than FPX_EPX_MK_MAX_PAIRS keys in one call: FPX_EINVAL, nothing applied.  Everything else is the
 * single-key form's contract, word for word.
 *
 * fpx_epx_preaccept_mk / _mk_dev / _mk_packed_dev: K5's tick.  When every command has exactly one key (key_offsets[i] = i)
 * the tick IS the single-key tick with keys as key (same kernels, same results, same device state).  Otherwise it runs
 * on (command, distinct key) pairs: each replica's pair sequence in its delivery order (an exclusive scan of the key
 * counts per replica), K5's sort / scan over the pairs, one max per command over its pairs' conflict rows, and K5's
 * decision on those rows (the output encoding is unchanged, so fpx_epx_execute_dev orders the commits as it does
 * single-key ones).  The device forms read key_offsets / keys on the device and wait once on the host for the pair count
 * (before anything is applied): not capturable into a HIP graph.  The multi-key tick never takes the on-chip
 * key-partitioned form (which decides per key).
 * fpx_epx_handle_preaccept_mk: K7 (fpx_epx_handle_preaccept) with the same pair expansion in array order.
 * fpx_epx_accept_mk / fpx_epx_handle_commit_mk: updateConflictIndex (Replica.scala:602-614) puts the instance under
 * every key of the command; no keys = nothing, as a Noop. */
#define FPX_EPX_MK_MAX_PAIRS (1 << 23)
int32_t fpx_epx_preaccept_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                             const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set,
                             const uint8_t* resp_mask, const uint8_t* seen_mask, const int32_t* rank,
                             const int32_t* triple_id, uint8_t* fast, int32_t* deps, int32_t* leader_deps,
                             int32_t* own_values_end);
int32_t fpx_epx_preaccept_mk_dev(fpx_epx* epx, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                 const int32_t* d_key_offsets, const int32_t* d_keys, const uint8_t* d_is_set,
                                 const uint8_t* d_resp_mask, const uint8_t* d_seen_mask, const int32_t* d_rank,
                                 const int32_t* d_triple_id, uint8_t* d_fast, int32_t* d_deps, int32_t* d_leader_deps,
                                 int32_t* d_own_values_end);
int32_t fpx_epx_preaccept_mk_packed_dev(fpx_epx* epx, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                        const int32_t* d_key_offsets, const int32_t* d_keys, const uint8_t* d_is_set,
                                        const uint8_t* d_resp_mask, const uint8_t* d_seen_mask, const int32_t* d_rank,
                                        const int32_t* d_triple_id, int32_t* d_packed);
int32_t fpx_epx_handle_preaccept_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                                    const int32_t* ballot_ordering, const int32_t* ballot_replica,
                                    const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set,
                                    const int32_t* triple_id, const int32_t* deps_in, const int32_t* deps_in_values_end,
                                    const uint8_t* target_mask, uint8_t* ok_bits, uint8_t* resend_bits,
                                    uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot, int32_t* reply_deps,
                                    int32_t* reply_values_end, int32_t* reply_triple);
int32_t fpx_epx_accept_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                          const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* triple_id,
                          const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set,
                          const uint8_t* target_mask, uint8_t* ok_bits, uint8_t* nack_bits, uint8_t* commit_bits,
                          int32_t* nack_ballot, uint8_t* committed);
int32_t fpx_epx_handle_commit_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number,
                                 const int32_t* triple_id, const int32_t* key_offsets, const int32_t* keys,
                                 const uint8_t* is_set, const int32_t* deps, const int32_t* deps_values_end,
                                 const uint8_t* target_mask);
/* ---- the leader half of an instance: hosted replicas that lead among peers in other processes ---------------------
 * FPX_EPX_F_LEADER_STATE in fpx_epx_config.flags (valid only with num_instances > 0, and n * n * num_instances <= 2^31;
 * FPX_EINVAL at fpx_epx_create otherwise): the context keeps Replica.leaderStates (epaxos/Replica.scala:499) per replica and
 * instance beside the command log -- the phase (none / PreAccepting / Accepting; Preparing with FPX_EPX_F_RECOVERY, below;
 * fpx_epx_prepare and fpx_epx_handle_prepare_oks stay the all-replicas-in-one-context form), the ballot, avoidFastPath, the triple id and the command's key / is_set, who has answered,
 * for PreAccepting every response's sequence number and dependencies, for Accepting the triple's.  16 + 4 n (n + 2) bytes
 * per (replica, leader, number): 76 / 156 / 268 B at n = 3 / 5 / 7, n * n * num_instances of them.  Without the flag nothing
 * of it is allocated, the three calls below are FPX_EINVAL and every other call behaves as it always did.
 *
 * The reference drops leaderStates(instance) when a PreAccept, Accept or Prepare of a higher ballot arrives (:1239-1242,
 * 1480-1483, 1645-1648) or the instance is committed (:831).  The kernels of those messages do not know about leader
 * state; in each of these cases the replica's own command-log entry ends committed or with a ballot above the one led in,
 * so a leader state is LIVE exactly while the entry at that replica is not committed and still carries the state's ballot
 * both as ballot and as vote ballot.  fpx_epx_leader_replies tests that (one gather per instance) before it looks at a
 * state; a state that is not live counts as none.  (fpx_epx_accept PROPOSED by the hosted replica itself in a higher ballot
 * -- a recovery it originates -- moves the entry the same way and so ends the state too, where the reference would replace
 * it by Accepting in the new ballot: a hosted replica among remote peers originates recovery with fpx_epx_recover instead.)
 *
 * fpx_epx_lead: transitionToPreAcceptPhase (:633-729) at ONE replica.  Message i: instance (leader[i], number[i]) led by
 *   replica at[i] in ballot (ballot_ordering[i], at[i]), command key[i] / is_set[i] (key -1 = Noop), CommandTriple id
 *   triple_id[i], avoidFastPath avoid_fast_path[i]; messages are handled in array order, instances pairwise distinct per
 *   call (FPX_EINVAL otherwise).  At replica at[i]: dependencies = the command's conflicts in THAT replica's index, in array
 *   order, minus the instance itself (:640-641, 569-600); PreAcceptedEntry(ballot, ballot, triple) (:684-693);
 *   updateConflictIndex (:694); leaderStates(instance) = PreAccepting with the replica's own PreAcceptOk, sequence number 0,
 *   as its first response (:712-728).  largestBallot is not touched (the reference does not touch it here).  It is K7's
 *   "processed" branch with an empty deps_in, on K7's scan.
 *   deps (m x n watermarks) / deps_values_end (m): the dependencies of the PreAccept to send, shaped like
 *   fpx_epx_handle_preaccept's deps_in (may be NULL).  A CommittedEntry at at[i], or an entry there with a larger ballot or
 *   vote ballot, is where the reference dies (:662-682): FPX_EFATAL_PROTOCOL, that message is skipped (its deps are zeros),
 *   the others are applied.  FPX_EINVAL with nothing applied and no output written: the flag missing, an instance outside the
 *   command log, a key outside the index (< -1 or >= num_keys), at[i] outside 0..n-1, ballot_ordering outside 0 .. 2^27 - 1.
 *   Single-key commands and Noops; key lists: fpx_epx_lead_mk.
 * fpx_epx_lead_mk: as fpx_epx_lead, with key lists (the CSR arrays and rules above FPX_EPX_MK_MAX_PAIRS; checked on the
 *   host).  The dependencies are the element-wise max over the command's distinct keys of each key's conflicts at replica
 *   at[i], and the put goes under every key (K7's pair form at one replica).  The leader state stores ONE key word: the key
 *   when the list has exactly one distinct key, -1 when it has none, FPX_EPX_KEY_LIST otherwise -- the caller holds the
 *   list by triple id.  One-key lists leave the outputs and the device state of fpx_epx_lead with key = keys. */
#define FPX_EPX_F_LEADER_STATE 1u
#define FPX_EPX_KEY_LIST (-2)
int32_t fpx_epx_lead(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                     const int32_t* ballot_ordering, const int32_t* key, const uint8_t* is_set, const int32_t* triple_id,
                     const uint8_t* avoid_fast_path, int32_t* deps, int32_t* deps_values_end);
int32_t fpx_epx_lead_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                        const int32_t* ballot_ordering, const int32_t* key_offsets, const int32_t* keys,
                        const uint8_t* is_set, const int32_t* triple_id, const uint8_t* avoid_fast_path, int32_t* deps,
                        int32_t* deps_values_end);
/* fpx_epx_leader_replies: ONE burst of what arrives at hosted leaders, in delivery order, the kinds interleaved, addressed
 * to any replica of the context, answered exactly as if handled one message at a time.  Message i: kind[i], to[i] the
 * receiving replica, the instance (leader[i], number[i]), the message's ballot (ballot_ordering[i], ballot_replica[i]) -- a
 * Nack's largest_ballot --, replica_index[i] the sender, and for a PreAcceptOk sequence_number[i] (NULL = zeros), deps[i * n ..]
 * (n watermarks) and deps_values_end[i] (NULL = zeros; the explicit ids number + 1 .. end - 1 of the own-leader column folded
 * into their end, 0 = none): the arrays of fpx_wire_epaxos_decode_replica_inbound plus who received each message.
 *   kind 0 PreAcceptOk (:1291-1419)  ignored unless the state is PreAccepting and the message's ballot is not below the
 *          state's; a ballot ABOVE it is logger.checkLt (:1333): FPX_EFATAL_PROTOCOL, the message is skipped.  Else
 *          responses(replicaIndex) = the message -- a later message of one sender replaces the earlier one, contents and
 *          all; replica_index == to replaces the leader's own response -- and with old / new the response counts:
 *            new < slowQuorumSize                                   FPX_EPX_WAITING (:1345)
 *            !avoidFastPath, old < slow <= new, slow < fast         FPX_EPX_START_SLOW_PATH_TIMER (:1353-1364)
 *            avoidFastPath (new >= slow)                            the slow path (:1369-1372)
 *            new >= fastQuorumSize                                  Util.popularItems over the (sequence number,
 *                     dependencies) of the senders other than `to`, threshold fastQuorumSize - 1 (:1382-1396): a
 *                     candidate -> FPX_EPX_FAST_COMMIT with it (:1401-1410), none -> the slow path (:1411-1415)
 *            anything else                                          FPX_EPX_WAITING
 *          the slow path (preAcceptingSlowPath :796-813, transitionToAcceptPhase :732-793): FPX_EPX_ACCEPT; the triple takes
 *          the max of the sequence numbers and the union of ALL responses' dependencies, the own one included;
 *          AcceptedEntry(ballot, ballot, triple) WITH its dependencies at `to`; the state becomes Accepting with the
 *          replica's own AcceptOk.
 *   kind 1 AcceptOk (:1514-1565)     ignored unless the state is Accepting and the ballot not below the state's; above it is
 *          logger.checkLt (:1550): FPX_EFATAL_PROTOCOL, skipped.  responses(replicaIndex) is set; slowQuorumSize of them ->
 *          FPX_EPX_SLOW_COMMIT with the Accept's triple, else FPX_EPX_WAITING.
 *   kind 2 Nack (:1577-1630)         largestBallot of `to` is raised in every case (:1578; fpx_epx_read_cmdlog's out[4]);
 *          FPX_EPX_NACK_RECOVER when an instance being led has a ballot < the Nack's (the caller starts or resets its
 *          recover-instance timer, :1623-1629), else FPX_EPX_NACK_IGNORED.
 *   kind 3 the defaultToSlowPath timer fired (:1015-1036), a caller event placed in the burst where it fired: state
 *          PreAccepting with at least slowQuorumSize responses -> the slow path, FPX_EPX_ACCEPT; any other state is the
 *          reference's logger.fatal (:1024-1028), fewer responses its logger.check (:801): FPX_EFATAL_PROTOCOL, skipped.
 *          The ballot, sender and dependency fields of a kind-3 message are not read.
 * Any commit writes CommittedEntry(triple) with its dependencies at `to` and clears the state (:815-831); the conflict index
 * already holds the instance (fpx_epx_lead put it, and TopOne.put is a maximum).  Dependencies are compared and united as
 * SETS: on the own-leader column of instance (L, x) a cover of x and a cover of x + 1 are the same set (the instance itself
 * is never a dependency, :582), so every response is brought to the form own_column gives before it is stored -- a
 * watermark above x with no explicit ids is read as a cover.
 * quorums (epaxos/Config.scala): slowQuorumSize = f + 1, fastQuorumSize = n - 1.
 * Outputs per message (any may be NULL): outcome; for FPX_EPX_FAST_COMMIT / _ACCEPT / _SLOW_COMMIT the triple of the Commit
 * or Accept the caller now sends -- out_seq, out_deps (m x n), out_values_end, out_triple (elsewhere 0 / zeros / 0 / -1);
 * decided_index[0 .. *num_decided) = the indices of those messages in message order, compacted on the device.  A message
 * that was skipped has outcome FPX_EPX_FATAL; the status is FPX_EFATAL_PROTOCOL and the rest of the burst is applied.
 * FPX_EINVAL, nothing applied, no output written: the flag missing, an unknown kind, `to` outside 0..n-1, an instance outside
 * the command log; for kinds 0 - 2 replica_index or ballot_replica outside 0..n-1 or ballot_ordering outside 0 .. 2^27 - 1;
 * for kind 0 a negative watermark or explicit ids not above the instance (deps_values_end != 0 needs
 * deps_values_end >= number + 2 and the own-leader watermark == number).  m < 2^30.
 * Cost: one stable radix sort of the burst on (to, leader, number) (K5's k_rs_*, up to three passes), then ONE thread per
 * instance walks that instance's messages in delivery order -- n - 1 of them in normal operation; k re-sent replies of one
 * instance are k sequential steps of one thread while the other instances proceed.
 * fpx_epx_leader_replies_dev: device pointers on the context's stream (d_num_decided too); status through fpx_epx_sync. */
enum {
  FPX_EPX_IGNORED = 0,               /* not leading / another phase / a stale ballot */
  FPX_EPX_WAITING = 1,               /* recorded; no quorum yet */
  FPX_EPX_START_SLOW_PATH_TIMER = 2, /* a slow quorum for the first time: start the defaultToSlowPath timer */
  FPX_EPX_FAST_COMMIT = 3,           /* commit(.., informOthers = true) on the fast path: send Commit */
  FPX_EPX_ACCEPT = 4,                /* transitionToAcceptPhase: send Accept to slowQuorumSize - 1 replicas */
  FPX_EPX_SLOW_COMMIT = 5,           /* commit of the Accept's triple: send Commit */
  FPX_EPX_NACK_RECOVER = 6,          /* start / reset the recover-instance timer */
  FPX_EPX_NACK_IGNORED = 7,
  FPX_EPX_FATAL = 8                  /* the reference would have died on this message; it was skipped */
};
int32_t fpx_epx_leader_replies(fpx_epx* epx, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                               const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                               const int32_t* replica_index, const int32_t* sequence_number, const int32_t* deps,
                               const int32_t* deps_values_end, int32_t* outcome, int32_t* out_seq, int32_t* out_deps,
                               int32_t* out_values_end, int32_t* out_triple, int32_t* decided_index, int32_t* num_decided);
int32_t fpx_epx_leader_replies_dev(fpx_epx* epx, int32_t m, const int32_t* d_kind, const int32_t* d_to,
                                   const int32_t* d_leader, const int32_t* d_number, const int32_t* d_ballot_ordering,
                                   const int32_t* d_ballot_replica, const int32_t* d_replica_index,
                                   const int32_t* d_sequence_number, const int32_t* d_deps, const int32_t* d_deps_values_end,
                                   int32_t* d_outcome, int32_t* d_out_seq, int32_t* d_out_deps, int32_t* d_out_values_end,
                                   int32_t* d_out_triple, int32_t* d_decided_index, int32_t* d_num_decided);
/* ---- the replica half of an instance, a burst at a time --------------------------------------------------------------
 * fpx_epx_replica_inbox: ONE burst of what peer replicas send hosted replicas -- PreAccept, Accept, Commit, Prepare -- in
 * delivery order, the kinds interleaved, instances and keys repeated freely, answered exactly as Replica.handlePreAccept /
 * handleAccept / handleCommit / handlePrepare would answer them one message at a time.  Needs num_instances > 0; does NOT
 * need FPX_EPX_F_LEADER_STATE.  Message i goes to the ONE replica to[i]: kind[i], the instance (leader[i], number[i]), the
 * message's ballot (ballot_ordering[i], ballot_replica[i]), the command key[i] / is_set[i] (key -1 = Noop; key lists:
 * fpx_epx_replica_inbox_mk), the CommandTriple's id triple_id[i], its dependencies deps[i * n ..] (n watermarks) and
 * deps_values_end[i] (the array may be NULL = zeros), shaped as fpx_epx_handle_preaccept's deps_in and
 * fpx_epx_handle_commit's deps.  For an Accept or a Commit deps[i * n] = -1 says "the triple is known by its id alone"
 * (what fpx_epx_read_cmdlog_deps reports for such an entry); the rest of that row is not read.
 *   kind FPX_EPX_IN_PRE_ACCEPT (:1159-1289), as fpx_epx_handle_preaccept at one replica:
 *          a CommittedEntry                                  FPX_EPX_RI_COMMIT_BACK, the Commit goes back (:1227-1238)
 *          an entry with ballot > the message's             FPX_EPX_RI_NACK (:1180-1184, 1189-1192, 1215-1218)
 *          PreAcceptedEntry voted in the message's ballot    FPX_EPX_RI_PRE_ACCEPT_OK_AGAIN, from the stored triple (:1196-1210)
 *          AcceptedEntry voted in the message's ballot       FPX_EPX_RI_IGNORED (:1222-1224)
 *          else                                              FPX_EPX_RI_PRE_ACCEPT_OK: largestBallot is raised (:1251), the
 *                 dependencies are the command's conflicts in to[i]'s index, minus the instance, united with the message's
 *                 (:1255-1262), PreAcceptedEntry(ballot, ballot, triple) (:1265-1276), updateConflictIndex (:1279)
 *   kind FPX_EPX_IN_ACCEPT (:1421-1511) -- handleAccept alone: no proposer step, no commit (fpx_epx_accept is the whole phase):
 *          a CommittedEntry                                  FPX_EPX_RI_COMMIT_BACK (:1463-1474)
 *          an entry with ballot > the message's             FPX_EPX_RI_NACK (:1432-1449)
 *          AcceptedEntry voted in the message's ballot       FPX_EPX_RI_ACCEPT_OK_AGAIN, nothing changes (:1451-1461)
 *          else                                              FPX_EPX_RI_ACCEPT_OK: largestBallot is raised (:1487),
 *                 AcceptedEntry(ballot, ballot, triple) with the message's dependencies, or by id (:1493-1502),
 *                 updateConflictIndex (:1503)
 *   kind FPX_EPX_IN_COMMIT (:1567-1575, 815-830): the entry is replaced whole by CommittedEntry(triple) with the message's
 *          dependencies (or by id), the index learns the command (:828): FPX_EPX_RI_LEARNT.  The ballot fields are not read.
 *   kind FPX_EPX_IN_PREPARE (:1632-1757): largestBallot is raised first, in every case (:1637).  The key fields are not read.
 *          a CommittedEntry                                  FPX_EPX_RI_COMMIT_BACK (:1744-1755)
 *          an entry with ballot > the message's             FPX_EPX_RI_NACK
 *          no entry / NoCommandEntry                         FPX_EPX_RI_PREPARE_OK, out_status 0, NoCommandEntry(ballot)
 *                                                            (:1654-1669, 1686-1701)
 *          else                                              FPX_EPX_RI_PREPARE_OK, out_status 2 (PreAccepted) / 3
 *                 (Accepted), out_ballot = the entry's voteBallot, the entry's triple; only `ballot` moves (:1711-1743)
 * A leader state of to[i] (FPX_EPX_F_LEADER_STATE) ends as the reference ends it (:1239-1242, 1480-1483, 1645-1648, 831):
 * every write of this call moves the entry as the per-kind calls do, and the liveness rule above fpx_epx_lead reads the entry.
 * Outputs per message (any may be NULL): outcome; out_ballot -- a Nack's largestBallot of to[i] AT THAT MOMENT of the burst
 * (encoded ordering * 8 + replica), a PrepareOk's voteBallot, else -1; out_status -- -1 unless FPX_EPX_RI_PREPARE_OK;
 * out_deps (m x n) / out_values_end / out_triple -- the dependencies and triple id of the reply that was sent: the
 * PreAcceptOk (first or again), the Commit sent back, the PrepareOk of status 2 / 3 (a triple stored by id: -1 in every
 * column); elsewhere zeros / 0 / -1.
 * FPX_EINVAL, nothing applied, no output written: num_instances = 0, an unknown kind, `to` outside 0..n-1, an instance
 * outside the command log; kinds 0, 1, 3: ballot_replica outside 0..n-1 or ballot_ordering outside 0 .. 2^27 - 1; kinds 0, 1,
 * 2: a key outside [-1, num_keys); kind 0: a negative watermark, an own-leader watermark above the instance, or explicit
 * ids not above it (deps_values_end != 0 needs the own-leader watermark == number and deps_values_end >= number + 2); kinds
 * 1, 2 with dependencies given: a negative watermark, or deps_values_end != 0 with deps_values_end <= number + 1 or the
 * own-leader watermark > number; m > FPX_EPX_INBOX_MAX; n * n * num_instances >= 2^32.  There is no FPX_EFATAL_PROTOCOL
 * on this side; m = 0 is FPX_OK.
 * Cost: one stable radix sort of the burst on (to, leader, number), ONE thread per (replica, instance) walking that cell's
 * messages in delivery order, then K7's conflict scan (a sort of n x m pairs on the key, one wavefront per (replica, key)) and
 * the largestBallot scan of fpx_epx_prepare.
 * fpx_epx_replica_inbox_dev: device pointers on the context's stream; status through fpx_epx_sync.
 *
 * fpx_epx_replica_inbox_mk / _mk_dev: as fpx_epx_replica_inbox / _dev, with key lists (the CSR arrays and rules above
 * FPX_EPX_MK_MAX_PAIRS) in place of key.  A Prepare's list is not looked up (the lists are one CSR: its offsets and keys are checked with the
 * rest).  An Accept taken in or a Commit puts the instance
 * under EVERY distinct key of its list (:602-614).  A processed PreAccept's conflicts are the element-wise max over its
 * distinct keys of each key's top-one row in to[i]'s index -- the puts to[i] made earlier in the burst and those from
 * before it -- and it then puts under every key.  One-key lists leave the outputs and the device state of
 * fpx_epx_replica_inbox with key = keys.  The device form also takes num_pairs, the length of d_keys: the lists are checked
 * on the device (d_key_offsets[0] = 0, non-decreasing, d_key_offsets[m] = num_pairs, keys in range), there is no host wait
 * for the pair count, and the status comes through fpx_epx_sync.  m <= FPX_EPX_INBOX_MAX, num_pairs <= FPX_EPX_MK_MAX_PAIRS.
 * Cost: the scan's sort is over n x num_pairs pairs, plus one max per processed PreAccept over its pairs' rows. */
#define FPX_EPX_INBOX_MAX (1 << 24)
enum { FPX_EPX_IN_PRE_ACCEPT = 0, FPX_EPX_IN_ACCEPT = 1, FPX_EPX_IN_COMMIT = 2, FPX_EPX_IN_PREPARE = 3 };
enum {
  FPX_EPX_RI_IGNORED = 0,
  FPX_EPX_RI_PRE_ACCEPT_OK = 1,       /* processed: send PreAcceptOk */
  FPX_EPX_RI_PRE_ACCEPT_OK_AGAIN = 2, /* send the PreAcceptOk of the stored triple again */
  FPX_EPX_RI_ACCEPT_OK = 3,           /* taken in: send AcceptOk */
  FPX_EPX_RI_ACCEPT_OK_AGAIN = 4,     /* send AcceptOk again */
  FPX_EPX_RI_LEARNT = 5,              /* a Commit: nothing to send */
  FPX_EPX_RI_PREPARE_OK = 6,          /* send PrepareOk(out_status, out_ballot, the triple) */
  FPX_EPX_RI_NACK = 7,                /* send Nack(instance, out_ballot) */
  FPX_EPX_RI_COMMIT_BACK = 8          /* the instance is committed here: send Commit with the stored triple */
};
int32_t fpx_epx_replica_inbox(fpx_epx* epx, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                              const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                              const int32_t* key, const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps,
                              const int32_t* deps_values_end, int32_t* outcome, int32_t* out_ballot, int32_t* out_status,
                              int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple);
int32_t fpx_epx_replica_inbox_dev(fpx_epx* epx, int32_t m, const int32_t* d_kind, const int32_t* d_to, const int32_t* d_leader,
                                  const int32_t* d_number, const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica,
                                  const int32_t* d_key, const uint8_t* d_is_set, const int32_t* d_triple_id,
                                  const int32_t* d_deps, const int32_t* d_deps_values_end, int32_t* d_outcome,
                                  int32_t* d_out_ballot, int32_t* d_out_status, int32_t* d_out_deps, int32_t* d_out_values_end,
                                  int32_t* d_out_triple);
int32_t fpx_epx_replica_inbox_mk(fpx_epx* epx, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                                 const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                                 const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set,
                                 const int32_t* triple_id, const int32_t* deps, const int32_t* deps_values_end,
                                 int32_t* outcome, int32_t* out_ballot, int32_t* out_status, int32_t* out_deps,
                                 int32_t* out_values_end, int32_t* out_triple);
int32_t fpx_epx_replica_inbox_mk_dev(fpx_epx* epx, int32_t m, const int32_t* d_kind, const int32_t* d_to,
                                     const int32_t* d_leader, const int32_t* d_number, const int32_t* d_ballot_ordering,
                                     const int32_t* d_ballot_replica, const int32_t* d_key_offsets, const int32_t* d_keys,
                                     int32_t num_pairs, const uint8_t* d_is_set, const int32_t* d_triple_id,
                                     const int32_t* d_deps, const int32_t* d_deps_values_end, int32_t* d_outcome,
                                     int32_t* d_out_ballot, int32_t* d_out_status, int32_t* d_out_deps,
                                     int32_t* d_out_values_end, int32_t* d_out_triple);
/* ---- the key table: equal key strings, equal key ids, on the device ------------------------------------------------------
 * Every entry point above takes key ids in [0, num_keys) and leaves the mapping from key strings to the caller; on the JVM
 * that is GpuEPaxosEngine.keyOf (jni/EPaxosNative.scala), a mutable.Map[String, Int].  A context that calls
 * fpx_epx_keys_enable keeps that map on the device (csrc/fpx_intern.hpp): an open-addressing table of
 * max(16, the power of two >= 2 x num_keys) slots under FNV-1a 64 with linear probing, the keys' bytes in an arena of
 * arena_bytes (< 2^31).  Opt-in: a context that never enables it is what it was.  A second call: FPX_EINVAL.
 *
 * fpx_epx_keys_intern: ONE batch of P strings, string p = bytes[off[p] .. off[p] + len[p]) -> ids[p].  Equal strings get
 * equal ids (keys are bytes, compared as bytes: no Unicode normalisation; the empty string is a key like any other); a
 * string the table does not hold gets the next id -- count, count + 1, ... in order of FIRST OCCURRENCE in the batch, so the
 * ids are a function of the input alone.  Ids are never reused and the table only grows.  Identity is always the byte
 * compare; the hash picks the home slot and nothing else.
 * FPX_EINVAL with nothing applied: a string outside the buffer or longer than FPX_EPX_KEY_MAX_LEN; P > FPX_EPX_MK_MAX_PAIRS;
 * a context without the table.  FPX_ECAPACITY with nothing applied (the same batch without its offender then succeeds):
 * more than num_keys distinct keys, or more than arena_bytes of them.  An error already raised on the context in front of
 * a _dev batch refuses it as well.  P = 0 is FPX_OK.
 * fpx_epx_keys_intern_dev: device pointers on the context's stream, no host wait; status through fpx_epx_sync; the ids
 * of a refused batch are -1.
 * fpx_epx_keys_count: the ids handed out and the arena bytes used (either may be NULL); waits for the stream.
 * fpx_epx_keys_read: ids first_id .. first_id + n - 1 back as bytes, for tests and for a JVM that warms its cache:
 * key_off_out[n + 1] (key j = bytes_out[key_off_out[j] .. key_off_out[j + 1])) and the bytes.  cap too small:
 * FPX_ECAPACITY with key_off_out filled, key_off_out[n] = the capacity needed (the convention of
 * fpx_wire_epaxos_decode_replica_inbound) -- call again.  Ids the table has not handed out: FPX_EINVAL. */
#define FPX_EPX_KEY_MAX_LEN 4096
int32_t fpx_epx_keys_enable(fpx_epx* epx, int64_t arena_bytes);
int32_t fpx_epx_keys_count(fpx_epx* epx, int32_t* count, int64_t* arena_used);
int32_t fpx_epx_keys_intern_dev(fpx_epx* epx, const uint8_t* d_bytes, int64_t bytes_len, const int64_t* d_off,
                                const int32_t* d_len, int32_t P, int32_t* d_ids);
int32_t fpx_epx_keys_intern(fpx_epx* epx, const uint8_t* bytes, int64_t bytes_len, const int64_t* off, const int32_t* len,
                            int32_t P, int32_t* ids);
int32_t fpx_epx_keys_read(fpx_epx* epx, int32_t first_id, int32_t n, int32_t* key_off_out, uint8_t* bytes_out, int64_t cap);
/* ---- the command store: a triple's serialised CommandOrNoop, by triple id, on the device ---------------------------------
 * The entry points above know a triple by its id alone; its bytes live with the caller (on the JVM, engine.triples of
 * jni/EPaxosNative.scala).  A context that calls fpx_epx_cmds_enable keeps them on the device as well (csrc/fpx_epx_cmds.hpp):
 * per triple id in [0, max_triples) a 64-bit arena offset (-1 = no bytes) and a length, and a byte arena of arena_bytes that
 * only grows -- the command log never forgets, and neither does the store.  With it the replies that carry a stored command
 * (the Commit sent back, the PrepareOk of a PreAccepted / Accepted instance) are encoded on the device
 * (include/fpx_wire.h).  Opt-in: a context that never enables it is what it was.  A second call, max_triples < 1 or a negative
 * size: FPX_EINVAL.
 *
 * fpx_epx_cmds_put: ONE burst of m records; record i's command is buf[cmd_off[i] .. cmd_off[i] + cmd_len[i]) and belongs to
 * triple triple_id[i].  Record i is considered only if triple_id[i] >= 0 and cmd_len[i] >= 0 (a Prepare has -1 in both).
 * The arena is a function of the input alone, whatever the schedule:
 *   - an id >= max_triples, or a length above FPX_EPX_CMD_MAX_LEN, is SKIPPED: counted, no error; the replies of such a
 *     triple stay deferred;
 *   - an id that has bytes already is left alone: first stored wins and nothing is compared (equal ids mean equal triples:
 *     that contract is the caller's, above);
 *   - among the records of the burst with a new id the lowest index is the writer;
 *   - the writers' commands are packed into the arena in index order, without padding;
 *   - new bytes that do not fit the free arena, or reach 4 GiB in one burst (the scan is 32 bits wide): nothing of the burst
 *     is stored, the burst counts as one REFUSED burst.  This is no context status: the call is FPX_OK.
 *   result[4]: new commands, new bytes, skipped records, refused (0 / 1).
 * FPX_EINVAL with nothing stored and nothing counted: a considered record whose (cmd_off, cmd_len) lies outside buf --
 * result is then {-1, the lowest such index, 0, 0}; a context without the store; m > FPX_EPX_INBOX_MAX; NULL arrays.
 * m = 0 is FPX_OK, result 0.
 * fpx_epx_cmds_put_dev: device pointers on the context's stream, no host wait; status through fpx_epx_sync.  A status
 * already raised on the context in front of it: it stands back, nothing stored, nothing counted, result 0.
 * fpx_epx_cmds_read: the bytes of one id into out[0 .. cap): *len = their number, -1 = the id has no bytes (FPX_OK);
 * *len > cap: FPX_ECAPACITY, call again.  An id outside [0, max_triples): FPX_EINVAL.  Waits for the stream.
 * fpx_epx_cmds_stats: out[4] = commands stored, arena bytes used, records skipped so far, bursts refused so far.
 * The copy has two forms (csrc/fpx_epx_cmds.hpp), the same bytes either way: lane l of a wavefront takes byte l, l + 64, ... of
 * its span (the default: the faster one on commands of tens of bytes, the A/B of profiles/epx_wire_replica_cmds.md), or, with
 * FPX_EPX_CMDS_WORDS in the environment of fpx_epx_create, aligned 16-byte words assembled from the unaligned source. */
#define FPX_EPX_CMD_MAX_LEN (1 << 16)
int32_t fpx_epx_cmds_enable(fpx_epx* epx, int32_t max_triples, int64_t arena_bytes);
int32_t fpx_epx_cmds_put_dev(fpx_epx* epx, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_cmd_off,
                             const int32_t* d_cmd_len, const int32_t* d_triple_id, int32_t m, int64_t* d_result);
int32_t fpx_epx_cmds_put(fpx_epx* epx, const uint8_t* buf, int64_t buf_len, const int64_t* cmd_off, const int32_t* cmd_len,
                         const int32_t* triple_id, int32_t m, int64_t* result);
int32_t fpx_epx_cmds_read(fpx_epx* epx, int32_t triple_id, uint8_t* out, int64_t cap, int32_t* len);
int32_t fpx_epx_cmds_stats(fpx_epx* epx, int64_t* out);
/* readback (parity) of one leader state: out[0] = phase (0 none, 1 PreAccepting, 2 Accepting, 3 Preparing; 0 when not live),
 * out[1] = ballot, out[2] = avoidFastPath, out[3] = triple id, out[4] = the key word as stored (the key; -1 for a Noop
 * or a command without keys; FPX_EPX_KEY_LIST for a list of two or more distinct keys), out[5] = is_set, out[6] = who has answered (bit
 * q), out[7] = the phase as stored (live or not); responses (may be NULL) n rows of n + 2 ints: row q = sequence number,
 * n watermarks, values_end of what replica q answered (meaningful for the bits of out[6]; Accepting: row `replica` holds
 * the triple's). */
int32_t fpx_epx_read_leader_state(fpx_epx* epx, int32_t replica, int32_t leader, int32_t number, int32_t out[8],
                                  int32_t* responses);
/* ---- originating an instance's recovery: the Preparing phase of a hosted replica among remote peers ------------------
 * FPX_EPX_F_RECOVERY in fpx_epx_config.flags, valid only together with FPX_EPX_F_LEADER_STATE (FPX_EINVAL at
 * fpx_epx_create otherwise).  The leader state gets a third phase, Preparing (3): per responder q the PrepareOk's status
 * (0 NotSeen, 2 PreAccepted, 3 Accepted -- fpx_epx_prepare's codes; 2 bits each in the state's head), its voteBallot and
 * triple id (a side array of 8 n bytes per cell: 24 / 40 / 56 B at n = 3 / 5 / 7) and its sequence number and
 * dependencies (the response row q that exists already, in canonical form).  Without the flag nothing of it is allocated
 * and the calls below are FPX_EINVAL.
 * LIVENESS extends the rule above fpx_epx_lead: a Preparing state is live exactly while the entry at that replica is not
 * committed and its `ballot` equals the state's.  The vote ballot is not compared: a Prepare moves `ballot` only.  Every
 * event on which the reference drops a Preparing state -- a higher-ballot PreAccept, Accept or Prepare (:1239-1242,
 * 1480-1483, 1645-1648), a commit (:831) -- raises the entry's ballot or commits it.
 *
 * fpx_epx_recover: transitionToPreparePhase (:969-996) at ONE hosted replica, with that replica's own Prepare.  Message i:
 *   the instance (leader[i], number[i]) at replica at[i]; array order; the instances of one call pairwise distinct.
 *   The ballot is Ballot(largestBallot(at).ordering + 1, at), which becomes largestBallot(at); the k-th recovery at one
 *   replica within a call takes ordering + k.  The reference sends the Prepare "to all replicas, including ourselves";
 *   the self-addressed one is delivered inside the call (one of its legal schedules), as handlePrepare (:1632-1757):
 *     a CommittedEntry                FPX_EPX_RV_COMMITTED, no state installed (the net effect of Prepare, the Commit
 *                                     back, and commit clearing the state); largestBallot stays raised
 *     no entry / NoCommandEntry       NoCommandEntry(ballot); the own PrepareOk has status 0
 *     else                            the entry's `ballot` moves; the own PrepareOk carries the entry's status,
 *                                     voteBallot, triple id and stored dependencies
 *   and in both of the latter FPX_EPX_RV_PREPARING: the state is Preparing in the new ballot with the own PrepareOk as
 *   its first response.  An entry whose ballot is not below the new one cannot occur (largestBallot bounds it); if it
 *   does: FPX_EPX_RV_FATAL, FPX_EFATAL_PROTOCOL, the message is skipped.
 *   Outputs (any may be NULL): outcome; out_ballot_ordering, the Prepare to send (ballot replica = at[i]); out_status /
 *   out_vote_ballot (encoded, -1 = null) / out_triple, the own PrepareOk (-1 where there is none).
 *   FPX_EINVAL, nothing applied: the flag missing, an instance outside the command log, at[i] outside 0..n-1, an instance
 *   repeated within the call, an ordering that would reach 2^27.
 *
 * fpx_epx_recovery_replies: ONE burst of PrepareOks in delivery order, addressed to any hosted replica, answered as
 *   handlePrepareOk (:1759-1869) would answer them one at a time.  Message i: to[i], the instance, the message's ballot,
 *   replica_index[i] the sender, status[i] (0 / 2 / 3), the voteBallot (vote_ballot_ordering[i], vote_ballot_replica[i];
 *   -1, -1 = null), triple_id[i] (equal commands carry equal ids, as everywhere a triple id is taken), and
 *   sequence_number[i] (NULL = zeros), deps[i * n ..], deps_values_end[i] (NULL = zeros) with the shape and validation of a
 *   PreAcceptOk of fpx_epx_leader_replies -- not read for status 0.  as_intended has fpx_epx_handle_prepare_oks' meaning:
 *   0 evaluates the two tests as the reference's code does (the Some(..) compare at :1813 never matches; :1836 reads the
 *   Prepare's ballot), 1 as its comments describe.
 *     the state not live or not Preparing, or a ballot below the state's      FPX_EPX_RC_IGNORED
 *     a ballot above the state's (checkLt :1792)      FPX_EPX_RC_FATAL, FPX_EFATAL_PROTOCOL, skipped, the rest applied
 *     else responses(replicaIndex) = the message (a later one of a sender replaces the earlier); fewer than f + 1
 *     responses                                       FPX_EPX_RC_WAITING
 *     at f + 1 the decision (:1804-1867), over the responses of the maximum voteBallot alone:
 *       as_intended only: an Accepted one                                   FPX_EPX_RC_ACCEPT with its triple
 *       as_intended only: Util.popularItems, threshold f, over the PreAccepted ones voted in Ballot(0, leader) from
 *         senders other than `to`, compared on (triple id, sequence number, dependencies AS SETS, by the own-column rule
 *         of fpx_epx_leader_replies): a candidate                           FPX_EPX_RC_ACCEPT with it
 *       a PreAccepted one                      FPX_EPX_RC_PRE_ACCEPT with its triple id
 *       else                                   FPX_EPX_RC_PRE_ACCEPT_NOOP
 *     out_source is the lowest replica index that qualifies (fpx_epx_handle_prepare_oks' choice), -1 for the Noop.
 *   A decision CLEARS the state; the transition itself is the caller's next call: fpx_epx_lead with the recovery's ballot
 *   ordering and avoid_fast_path = 1 for RC_PRE_ACCEPT (the command filed under the triple id) and RC_PRE_ACCEPT_NOOP (key
 *   -1), fpx_epx_lead_accept for RC_ACCEPT.
 *   ORDERING CONTRACT: the caller applies a burst's decisions before it hands the context another burst of any kind for
 *   those instances.  Between the two calls the state is none, where the reference moved atomically.
 *   Outputs per message (any may be NULL): outcome, out_source, out_triple (-1 without one), out_ballot (the recovery's
 *   ballot, encoded, on a decision; else -1), for RC_ACCEPT the triple's out_seq / out_deps (m x n) / out_values_end
 *   (elsewhere zeros; an own PrepareOk whose entry knew its triple by id alone gives -1 in every column);
 *   decided_index[0 .. *num_decided) = the indices of the decisions in message order, compacted on the device.
 *   FPX_EINVAL, nothing applied, no output written: the flag missing, an index or ballot out of range, a status outside
 *   {0, 2, 3}, malformed dependencies of a status-2/3 message, m >= 2^30.  m = 0 is FPX_OK.
 * fpx_epx_recovery_replies_dev: device pointers on the context's stream (d_num_decided too); status through fpx_epx_sync.
 *
 * fpx_epx_lead_accept: transitionToAcceptPhase (:732-793) at ONE hosted replica with a triple the caller names; host
 *   pointers, array order, instances pairwise distinct.  A CommittedEntry at at[i], or an entry there with a larger ballot
 *   or vote ballot, is the reference's fatal / checkLe: FPX_EFATAL_PROTOCOL, the message is skipped.  Else
 *   AcceptedEntry(ballot, ballot, triple) with the given dependencies (deps[i * n] = -1: by id alone, as an Accept of
 *   fpx_epx_replica_inbox), updateConflictIndex (the replica may never have seen the instance), and the state becomes
 *   Accepting with the replica's own AcceptOk and the triple in row at[i].  largestBallot is not touched.  The AcceptOks
 *   then go through fpx_epx_leader_replies unchanged.  FPX_EINVAL as fpx_epx_lead, and for dependencies an Accept of the
 *   inbox would refuse.
 * fpx_epx_lead_accept_mk: as fpx_epx_lead_accept, with key lists (checked on the host): updateConflictIndex puts the
 *   instance under every key, and the state's key word follows fpx_epx_lead_mk's rule.
 * fpx_epx_read_leader_state reports out[0] = 3 for a live Preparing state; its responses rows are the PrepareOks'
 * (sequence number, dependencies).  fpx_epx_read_recovery_state: out n x 3 = per responder status, voteBallot (encoded),
 * triple id; -1, -1, -1 for a replica that has not answered or when the stored phase is not Preparing. */
#define FPX_EPX_F_RECOVERY 2u
enum { FPX_EPX_RV_PREPARING = 0, FPX_EPX_RV_COMMITTED = 1, FPX_EPX_RV_FATAL = 2 };
enum {
  FPX_EPX_RC_IGNORED = 0,
  FPX_EPX_RC_WAITING = 1,
  FPX_EPX_RC_ACCEPT = 2,          /* fpx_epx_lead_accept with the triple given */
  FPX_EPX_RC_PRE_ACCEPT = 3,      /* fpx_epx_lead, avoid_fast_path = 1, the command of out_triple */
  FPX_EPX_RC_PRE_ACCEPT_NOOP = 4, /* fpx_epx_lead, avoid_fast_path = 1, a Noop */
  FPX_EPX_RC_FATAL = 5            /* the reference would have died on this message; it was skipped */
};
int32_t fpx_epx_recover(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                        int32_t* outcome, int32_t* out_ballot_ordering, int32_t* out_status, int32_t* out_vote_ballot,
                        int32_t* out_triple);
int32_t fpx_epx_recovery_replies(fpx_epx* epx, int32_t m, const int32_t* to, const int32_t* leader, const int32_t* number,
                                 const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* replica_index,
                                 const int32_t* status, const int32_t* vote_ballot_ordering,
                                 const int32_t* vote_ballot_replica, const int32_t* triple_id, const int32_t* sequence_number,
                                 const int32_t* deps, const int32_t* deps_values_end, int32_t as_intended, int32_t* outcome,
                                 int32_t* out_source, int32_t* out_triple, int32_t* out_ballot, int32_t* out_seq,
                                 int32_t* out_deps, int32_t* out_values_end, int32_t* decided_index, int32_t* num_decided);
int32_t fpx_epx_recovery_replies_dev(fpx_epx* epx, int32_t m, const int32_t* d_to, const int32_t* d_leader,
                                     const int32_t* d_number, const int32_t* d_ballot_ordering,
                                     const int32_t* d_ballot_replica, const int32_t* d_replica_index, const int32_t* d_status,
                                     const int32_t* d_vote_ballot_ordering, const int32_t* d_vote_ballot_replica,
                                     const int32_t* d_triple_id, const int32_t* d_sequence_number, const int32_t* d_deps,
                                     const int32_t* d_deps_values_end, int32_t as_intended, int32_t* d_outcome,
                                     int32_t* d_out_source, int32_t* d_out_triple, int32_t* d_out_ballot, int32_t* d_out_seq,
                                     int32_t* d_out_deps, int32_t* d_out_values_end, int32_t* d_decided_index,
                                     int32_t* d_num_decided);
int32_t fpx_epx_lead_accept(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                            const int32_t* ballot_ordering, const int32_t* key, const uint8_t* is_set,
                            const int32_t* triple_id, const int32_t* sequence_number, const int32_t* deps,
                            const int32_t* deps_values_end);
int32_t fpx_epx_lead_accept_mk(fpx_epx* epx, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                               const int32_t* ballot_ordering, const int32_t* key_offsets, const int32_t* keys,
                               const uint8_t* is_set, const int32_t* triple_id, const int32_t* sequence_number,
                               const int32_t* deps, const int32_t* deps_values_end);
int32_t fpx_epx_read_recovery_state(fpx_epx* epx, int32_t replica, int32_t leader, int32_t number, int32_t* out);
/* one command-log entry: out[0..4] = kind, ballot, voteBallot, triple id, the replica's largestBallot */
int32_t fpx_epx_read_cmdlog(fpx_epx* epx, int32_t replica, int32_t leader, int32_t number, int32_t out[5]);
/* the dependencies kept with that entry: deps[n] watermarks (deps[0] = -1: known by triple id only), *values_end */
int32_t fpx_epx_read_cmdlog_deps(fpx_epx* epx, int32_t replica, int32_t leader, int32_t number, int32_t* deps,
                                 int32_t* values_end);
/* replica's conflict-index entry of one key: gets[n], sets[n] (TopOne vectors) */
int32_t fpx_epx_read_index(fpx_epx* epx, int32_t replica, int32_t key, int32_t* gets, int32_t* sets);

/* ---- next rows of SURVEY.md section 8(f) ----------------------------------------------------------
 *
 * f1  Replica.handleChosen + executeLog (multipaxos/Replica.scala:572-590, 394-447;
 *     util/BufferMap.scala:29-51): the receiver of Chosen.  One replica log per context (every replica
 *     receives the same Chosen stream).  For i in order with mask[i] != 0 (mask NULL = all):
 *     log.get(slot) defined -> ignored (redundantly chosen); else log.put(slot, value), numChosen += 1;
 *     then the contiguous prefix executes: executedWatermark advances while log.get(it) is defined.
 *     Outputs (may be NULL): the new executedWatermark and numChosen. */
int32_t fpx_replica_chosen(fpx_ctx* ctx, int32_t n, const int32_t* slot, const int32_t* value_id,
                           const uint8_t* mask, int32_t* executed_watermark, int32_t* num_chosen);
/* device-resident inputs; the result is read with fpx_replica_state after fpx_sync */
int32_t fpx_replica_chosen_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot,
                               const int32_t* d_value_id, const uint8_t* d_mask);
int32_t fpx_replica_state(fpx_ctx* ctx, int32_t* executed_watermark, int32_t* num_chosen);
/* mencius.Replica.handleChosenNoopRange (mencius/Replica.scala:464-485): the slots slot_start,
 * slot_start + num_leader_groups, ... below slot_end are put as Noop in order until the first one that is
 * ALREADY in the log -- there the reference handler returns: the rest of the range is dropped and
 * executeLog does not run (kept as is).  Otherwise the contiguous prefix executes.  Synchronous. */
int32_t fpx_replica_chosen_noop_range(fpx_ctx* ctx, int32_t slot_start, int32_t slot_end,
                                      int32_t* executed_watermark, int32_t* num_chosen);
/* mencius.Replica.handleChosen + handleChosenNoopRange (mencius/Replica.scala:402-420, 464-485; executeLog :331-371) for
 * a BURST of n messages in delivery order, the two kinds interleaved as a Mencius replica's inbox has them (:380-400).
 * kind[i] (fpx_wire.h): FPX_WIRE_CHOSEN = Chosen(slot[i], value_id[i]); FPX_WIRE_CHOSEN_NOOP_RANGE =
 * ChosenNoopRange(slot[i], slot_end[i]) (value_id[i] is ignored); any other kind, and any message with mask[i] == 0
 * (mask may be NULL), is skipped -- the arrays are what fpx_wire_mencius_decode_replica_inbound produces.  The result is
 * EXACTLY the state after handling the messages one by one:
 *   Chosen: slot in the log -> ignored and executeLog does NOT run (here fpx_replica_chosen[_dev], which always scans,
 *     differs); else put, numChosen += 1, executeLog.
 *   ChosenNoopRange: slot, slot + num_leader_groups, ... below slot_end in order: the first one that is in the log ends the
 *     handler (the rest is dropped, executeLog does not run); the others get Noop (-1), numChosen += 1.  A range that runs
 *     to its end (an empty one included) runs executeLog.
 * So the lower index puts a slot; a range is cut by what an earlier message of the same burst put, not by a later one; and
 * executedWatermark is the contiguous prefix of the log as it stood after the last message that reached executeLog (it
 * does not move when none did), while numChosen counts every put.
 * _dev: device pointers, enqueued on the context's stream, nothing is read by the host between its passes; read the
 * result with fpx_replica_state / fpx_replica_read_log.  A Chosen with a slot outside [0, num_slots), or a range with
 * slot < 0 or slot_end > num_slots, is found on the device before anything is applied: FPX_EINVAL at fpx_sync, the lowest
 * offending index in fpx_error_detail, log and scalars untouched.  NULL context, n < 0 or n >= 2^30, or a NULL d_kind /
 * d_slot / d_slot_end / d_value_id with n > 0: FPX_EINVAL at once, nothing enqueued.  The first call allocates one int32
 * per slot (4 B x num_slots, kept until fpx_destroy, counted by fpx_device_bytes).
 * One array per field, the two kinds in the same arrays, so that a band feeds the call without a copy: a caller that lays
 * out d_slot | d_slot_start in one buffer, d_chosen | d_range_chosen in one buffer, and gives d_chosen_value n_ranges
 * spare words passes fpx_mencius_band_fused_dev's outputs straight in as d_slot, d_mask and d_value_id, with constant
 * d_kind / d_slot_end arrays.
 * The host form takes host arrays, any n, and is synchronous (outputs may be NULL). */
int32_t fpx_replica_chosen_msgs_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_slot,
                                    const int32_t* d_slot_end, const int32_t* d_value_id, const uint8_t* d_mask);
int32_t fpx_replica_chosen_msgs(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* slot,
                                const int32_t* slot_end, const int32_t* value_id, const uint8_t* mask,
                                int32_t* executed_watermark, int32_t* num_chosen);
/* multipaxos.Replica's inbox (multipaxos/Replica.scala): handleChosen + executeLog (:572-590, 394-413) and the read path,
 * handleDeferrableRead[s] / processDeferredReads / executeRead and the eventual reads (:455-529, 629-690), for a BURST of n
 * messages in delivery order.  kind[i] (fpx_wire.h): FPX_WIRE_CHOSEN = Chosen(slot[i], value_id[i]); a DEFERRABLE read =
 * FPX_WIRE_READ_REQUEST / SEQUENTIAL_READ_REQUEST / READ_REQUEST_BATCH / SEQUENTIAL_READ_REQUEST_BATCH with the request's
 * slot in slot[i] (any int32: -1 is what a read batcher sends, negative means "at once"); an EVENTUAL read =
 * FPX_WIRE_EVENTUAL_READ_REQUEST[_BATCH] (slot[i] is ignored).  value_id[i] is read for Chosens only.  Any other kind, and
 * any message with mask[i] == 0 (mask may be NULL), is skipped.  A batch is ONE message: its commands share one slot and
 * one fate.  With W0 = executedWatermark before the burst, W(i) = the watermark after the messages < i and W1 = the
 * watermark after the burst, the result is EXACTLY that of handling the messages one by one:
 *   Chosen: as fpx_replica_chosen_msgs handles a Chosen -- the lower index puts a slot, a slot that is in the log already
 *     is ignored, numChosen counts the puts; the log, numChosen and executedWatermark end as they do there.
 *   eventual read at i: runs at once: exec_count[i] = W(i), reply_slot[i] = W(i) - 1.
 *   deferrable read at i with slot r: r < W(i): at once, as above.  Otherwise it is deferred under r.  r < W1: it is
 *     released in this burst, inside the executeLog that executes slot r, after that slot's commands and before the next
 *     slot's: exec_count[i] = r + 1 and reply_slot[i] = r - 1.  That reply slot is the reference's as it evaluates it, kept
 *     as is: executeRead reads executedWatermark - 1 while executeLog has not yet incremented the watermark past r
 *     (:405-413, 526), so a released read reports one slot less than the same read would have reported had it arrived
 *     right after the Chosen.  r >= W1 (r >= num_slots included): still deferred, exec_count[i] = reply_slot[i] = -1.
 *   anything that is not a read (Chosens, skipped messages): exec_count[i] = reply_slot[i] = -2.
 * exec_count is the number of log entries executed before the read runs.  order: first the indices of the reads that run in
 * this burst, in the order the reference runs them = ascending (exec_count, index) (the reads deferred under r all arrived
 * before the message that executed r, the reads that ran at once with exec_count r + 1 all after it), then the reads still
 * deferred in index order; only its first counts[0] entries are written.  counts[4] = the number of reads, the number that
 * ran, W0, W1.  The caller runs its state machine over slots W0 .. W1 - 1, interleaving the reads by exec_count, and hands
 * the still-deferred reads back at the FRONT of its next burst in the order `order` lists them: the call keeps no read
 * state between bursts, and because the watermark does not move between calls they defer again, ahead of every newer read
 * of their slot -- re-submission is exact.
 * MultiPaxos contexts only: num_leader_groups > 1 is FPX_EINVAL at once (mencius.Replica has no read handlers).
 * _dev: device pointers (arrays of n; d_counts of 4), enqueued on the context's stream, nothing is read by the host
 * between its passes.  A Chosen with a slot outside [0, num_slots) is found on the device before anything is applied:
 * FPX_EINVAL at fpx_sync, the lowest offending index in fpx_error_detail, log and scalars untouched, no output written.
 * The four outputs may be NULL together (some but not all: FPX_EINVAL): then the call is fpx_replica_chosen_msgs_dev for
 * a burst without ranges.  NULL context, n < 0 or n >= 2^30, or a NULL d_kind / d_slot / d_value_id with n > 0:
 * FPX_EINVAL at once, nothing enqueued.  The claim words are fpx_replica_chosen_msgs_dev's (4 B x num_slots); the call's
 * scratch (4 B per 256 slots and about 17 B per message) lives in the context, is allocated on first use, grows with n and
 * is counted by fpx_device_bytes.
 * The host form takes host arrays, any n, and is synchronous; exec_count, reply_slot and order (n > 0) and counts are
 * required there, executed_watermark and num_chosen may be NULL; on an error the output arrays are left untouched. */
int32_t fpx_replica_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_slot,
                              const int32_t* d_value_id, const uint8_t* d_mask, int32_t* d_exec_count,
                              int32_t* d_reply_slot, int32_t* d_order, int32_t* d_counts);
int32_t fpx_replica_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* slot, const int32_t* value_id,
                          const uint8_t* mask, int32_t* exec_count, int32_t* reply_slot, int32_t* order,
                          int32_t counts[4], int32_t* executed_watermark, int32_t* num_chosen);
/* multipaxos.Acceptor's inbox (multipaxos/Acceptor.scala:122-254): handlePhase1a (:148-182), handlePhase2a (:184-220),
 * handleMaxSlotRequest (:222-237) and handleBatchMaxSlotRequest (:239-254) for a BURST of n AcceptorInbound messages in
 * delivery order, the kinds interleaved and addressed to any of the context's acceptors -- what a reference ProxyLeader
 * (one Phase2a per acceptor address, to f + 1 of them, multipaxos/ProxyLeader.scala:190-215), Leader, Client and
 * ReadBatcher send.  The mirror image of fpx_proxy_phase2b_msgs: NO run contract applies -- a slot may come any number of
 * times, rounds may go up and down.  The arrays are what fpx_wire_decode_acceptor_inbound[_dev] produces, plus who
 * received each message:
 *   kind[i] (fpx_wire.h): FPX_WIRE_PHASE2A (slot, round, value_id) / FPX_WIRE_PHASE1A (round) / FPX_WIRE_MAX_SLOT_REQUEST /
 *     FPX_WIRE_BATCH_MAX_SLOT_REQUEST (slot, round and value_id are not read: the decoder keeps other fields there);
 *     FPX_WIRE_OTHER is skipped (none of its fields is read).
 *   group_index[i] (NULL = 0), acceptor_index[i]: the acceptor the message was delivered to, LOCAL to the context:
 *     grid_cols == 0: acceptor acceptor_index (0 .. num_replicas - 1) of acceptor group group_index (0 .. num_groups - 1);
 *     grid_cols > 0: acceptor group_index * grid_cols + acceptor_index of the context's one group, as in
 *     fpx_proxy_phase2b_msgs.
 * The result is EXACTLY that of every acceptor handling its messages one by one in index order.  For acceptor e:
 *   Phase2a / Phase1a with round[i] < e.round: Nack(e.round) (:155, :192 -- `<`: an equal round is accepted again).
 *   otherwise e.round := round[i]; a Phase2a stores (round[i], value_id[i]) in cell (slot[i], e) and raises maxVotedSlot
 *     (:204-209).  The cell keeps the LAST accepted Phase2a of (e, slot) in the burst, an equal round sent again with
 *     another value included.
 *   MaxSlotRequest / BatchMaxSlotRequest: answered with e.maxVotedSlot as it stands at that message (:233, :250).
 * reply_kind[i]: 0 = no reply (skipped), FPX_WIRE_PHASE2B = voted, FPX_WIRE_NACK, FPX_WIRE_PHASE1B = promised,
 * FPX_WIRE_MAX_SLOT_REQUEST = answered.  reply_value[i]: a Nack's round (the acceptor's, at that moment); a vote's or a
 * promise's round (the message's); a read's maxVotedSlot; -1 with no reply.  A Nack goes to
 * fpx_round_leader(num_leaders, round[i]) (:197), which stays with the caller.  Either output may be NULL.
 * Afterwards the acceptors' rounds, maxVotedSlots and vote cells (fpx_read_scalars, fpx_read_state, fpx_state_digest) are
 * what the message-at-a-time route (fpx_acceptor_phase2a / fpx_acceptor_phase1a with single-bit masks) leaves, and so is
 * what the vote kernels keep about fresh rows.
 * Phase1b.info is NOT produced: the call moves rounds and reports promise or Nack.  A promise's info is the acceptor's
 * votes as of that message (:167-180), so a caller that needs it ends its burst at that Phase1a and calls
 * fpx_acceptor_phase1b_info_all[_dev] for the promisers (jni/Native.scala's GpuAcceptor does).  A Phase1a in the middle
 * of a burst is still handled correctly for every later message.
 * FPX_BALLOT_ACCEPTOR contexts with num_leader_groups == 1 only (Mencius acceptors: fpx_mencius_acceptor_inbox below);
 * with grid_cols > 0, num_groups == 1: anything else, a
 * NULL context, n < 0 or n >= 2^30, grid_cols < 0, or a NULL kind / acceptor_index / slot / round / value_id with n > 0
 * is FPX_EINVAL at once, nothing enqueued.  n == 0 is FPX_OK.
 * _dev: device pointers (arrays of n), enqueued on the context's stream behind the fold of an earlier fused step
 * (fpx_deferred_folds); nothing is read by the host between its passes (csrc/fpx_acceptor_inbox.hpp: a stable radix
 * sort by acceptor, two device-wide running maxima, a claim table sized by the burst; integer atomics only, results are
 * reproducible).  A kind other than the five above, an index that names no acceptor of the context, and for a
 * Phase2a / Phase1a a round outside 0 .. 2^30 - 2, for a Phase2a a slot outside [0, num_slots) or of another acceptor
 * group than the message's, are found on the device before anything is applied: FPX_EINVAL at fpx_sync, the LOWEST
 * offending index in fpx_error_detail, state untouched, no output written, and (the _dev convention) the context applies
 * nothing up to that fpx_sync.  The scratch (about 40 B per message and a claim table of 12 B x the power of two at or
 * above 2 n) lives in the context, is allocated on first use, grows with n and is counted by fpx_device_bytes.
 * The host form takes host arrays, goes through the staging driver as a single run and is synchronous; on an error the
 * output arrays are left untouched. */
int32_t fpx_acceptor_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                               const int32_t* d_acceptor_index, const int32_t* d_slot, const int32_t* d_round,
                               const int32_t* d_value_id, int32_t grid_cols, int32_t* d_reply_kind,
                               int32_t* d_reply_value);
int32_t fpx_acceptor_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                           const int32_t* acceptor_index, const int32_t* slot, const int32_t* round,
                           const int32_t* value_id, int32_t grid_cols, int32_t* reply_kind, int32_t* reply_value);
/* mencius.Acceptor's inbox (mencius/Acceptor.scala:142-291): handlePhase1a (:166-200), handlePhase2a (:202-235) and
 * handlePhase2aNoopRange (:237-291) for a BURST of n AcceptorInbound messages in delivery order, the kinds interleaved and
 * addressed to any of the context's acceptors -- what reference mencius.ProxyLeaders send: one Phase2a per acceptor
 * address to quorumSize acceptors of the slot's group, one Phase2aNoopRange per acceptor address to quorumSize acceptors
 * of every acceptor group of the leader group (mencius/ProxyLeader.scala:216-303).  The Mencius form of
 * fpx_acceptor_inbox: NO run contract applies.  The arrays are what fpx_wire_mencius_decode_acceptor_inbound produces,
 * plus who received each message:
 *   kind[i] (fpx_wire.h): FPX_WIRE_PHASE2A (slot, round, value_id) / FPX_WIRE_PHASE2A_NOOP_RANGE (slot = start inclusive,
 *     slot_end = end exclusive, round) / FPX_WIRE_PHASE1A (round); FPX_WIRE_OTHER is skipped (none of its fields is
 *     read).  mencius.Acceptor has no read path: the two MaxSlotRequest kinds are a bad kind here.
 *   group_index[i] (NULL = 0): leader_group * num_groups + acceptor_group, the row numbering of fpx_read_scalars;
 *   acceptor_index[i]: the acceptor inside that group (0 .. num_replicas - 1), LOCAL to the context.
 * The result is EXACTLY that of every acceptor handling its messages one by one in index order.  For acceptor e:
 *   a message of any of the three kinds with round[i] < e.round: Nack(e.round) (:173, :210, :245 -- `<`: an equal round is
 *     accepted again).
 *   otherwise e.round := round[i]; a Phase2a stores (round, value_id) in cell (slot, e); a range stores (round, Noop = -1)
 *     in cell (s, e) of every s in [start, end) with s = start (mod L) and (s / L) % A == e's acceptor group (:261-277).
 *     The start need not be a slot of e's acceptor group, a range may own no slot at all, and an empty range still moves
 *     the round and is still answered.
 *   every cell ends as its LAST accepted covering message left it, a point or a range, whatever their rounds (equal
 *     rounds with different values come out in index order).
 *   max_voted (the scalar the library keeps in every mode) is raised by a Phase2a's slot and by a range's largest owned
 *     slot, as fpx_acceptor_phase2a / fpx_acceptor_phase2a_noop_range raise it.
 * reply_kind[i]: 0 = no reply (skipped), FPX_WIRE_PHASE2B, FPX_WIRE_PHASE2B_NOOP_RANGE, FPX_WIRE_PHASE1B = promised,
 * FPX_WIRE_NACK.  reply_value[i]: a Nack's round (the acceptor's, at that moment); a vote's or a promise's round (the
 * message's); -1 with no reply.  A Nack goes to leader fpx_round_leader(num_leaders, round[i]) of leader group
 * slot % L / start % L (:215-218, :250-253), which stays with the caller.  Either output may be NULL.
 * Afterwards the acceptors' rounds, max_voted and vote cells (fpx_read_scalars, fpx_read_state, fpx_state_digest) are what
 * the message-at-a-time route (fpx_acceptor_phase2a / fpx_acceptor_phase2a_noop_range / fpx_acceptor_phase1a with
 * single-bit masks) leaves, and so is what the vote kernels keep about fresh rows.
 * Phase1b.info is NOT produced, as in fpx_acceptor_inbox: a caller that needs it ends its burst at that Phase1a and calls
 * fpx_acceptor_phase1b_info_all[_dev] for the promisers (jni/MenciusNative.scala's GpuMenciusEngine does).
 * FPX_BALLOT_ACCEPTOR contexts without a grid quorum (num_leader_groups == 1 is allowed): anything else, a NULL context,
 * n < 0 or n >= 2^30, or a NULL kind / acceptor_index / slot / slot_end / round / value_id with n > 0 is FPX_EINVAL at
 * once, nothing enqueued.  n == 0 is FPX_OK.
 * _dev: device pointers (arrays of n), enqueued on the context's stream behind the fold of an earlier fused step
 * (fpx_deferred_folds); nothing is read by the host between its passes (csrc/fpx_mencius_acceptor_inbox.hpp: the sort and
 * the running maxima of fpx_acceptor_inbox, the accepted ranges compacted into a list, every cell written by exactly one
 * thread; integer atomics only, results are reproducible).  Another kind, an index that names no acceptor of the
 * context, a round outside 0 .. 2^30 - 2, a Phase2a slot outside [0, num_slots) or of another group than the message's,
 * a range with start < 0, end < start or end > num_slots, and a range whose start % L is not the receiving acceptor's
 * leader group (its cells lie in rows that acceptor has no column in) are found on the device before anything is
 * applied: FPX_EINVAL at fpx_sync, the LOWEST offending index in fpx_error_detail, state untouched, no output written,
 * and (the _dev convention) the context applies nothing up to that fpx_sync.  The scratch (about 64 B per message and
 * fpx_acceptor_inbox's claim table) lives in the context, is allocated on first use, grows with n and is counted by
 * fpx_device_bytes.  Settling the cells costs (owned cells of a range) x (later accepted ranges of the same acceptor in
 * the burst) interval tests: meant for the handful of ranges per acceptor a tick carries.
 * The host form takes host arrays, goes through the staging driver as a single run and is synchronous; on an error the
 * output arrays are left untouched. */
int32_t fpx_mencius_acceptor_inbox_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_kind, const int32_t* d_group_index,
                                       const int32_t* d_acceptor_index, const int32_t* d_slot,
                                       const int32_t* d_slot_end, const int32_t* d_round, const int32_t* d_value_id,
                                       int32_t* d_reply_kind, int32_t* d_reply_value);
int32_t fpx_mencius_acceptor_inbox(fpx_ctx* ctx, int32_t n, const int32_t* kind, const int32_t* group_index,
                                   const int32_t* acceptor_index, const int32_t* slot, const int32_t* slot_end,
                                   const int32_t* round, const int32_t* value_id, int32_t* reply_kind,
                                   int32_t* reply_value);
/* log entries [first, first + count): value (-1 where absent) and present flag */
int32_t fpx_replica_read_log(fpx_ctx* ctx, int32_t first, int32_t count, int32_t* values,
                             uint8_t* present);

/* f2  Leader.handlePhase1b recovery scan (multipaxos/Leader.scala:306-329 safeValue, :543-566).
 *     quorum_masks: one 4-word set per acceptor group (num_leader_groups * num_groups x 4): the
 *     acceptors whose Phase1b the leader holds.  maxSlot = the largest slot >= chosen_watermark in
 *     which any of them voted (-1 if none).  For slot = chosen_watermark .. maxSlot (at most cap
 *     entries are written): safe_round = the highest voteRound among the quorum's acceptors of the
 *     slot's group that voted in the slot (-1 if none voted), safe_value = the value voted in that
 *     round (FPX_NOOP if none: "everything is safe, we return Noop"; when several of them voted in
 *     that round, the value of the one with the lowest index).  Only the bits [replica_base,
 *     replica_base + num_replicas) of a set are read: a bit outside them names no acceptor of this
 *     context and is ignored, it is not an error. */
int32_t fpx_leader_phase1b_scan(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* quorum_masks,
                                int32_t cap, int32_t* max_slot, int32_t* safe_round,
                                int32_t* safe_value);

/* Leader.handlePhase1b (multipaxos/Leader.scala:306-329, 504-577; mencius/Leader.scala:359-385, 582-659) for a BURST of
 * n Phase1b MESSAGES in delivery order -- the acceptors anywhere: reference processes (the outputs of
 * fpx_wire_decode_leader_inbound), other contexts or GPUs of a replica-sharded group (the outputs of
 * fpx_acceptor_phase1b_info_all_dev, as they stand).  Stateless with respect to Phase 1: the context gives the geometry
 * (num_groups, num_leader_groups, f, replicas_total, the read-quorum predicate) and keeps the scratch; no acceptor, tally
 * or replica state is read or written.  A caller still waiting for a quorum calls again with the longer burst.
 * Message i: kind[i] (NULL = every message is a Phase1b; kinds other than FPX_WIRE_PHASE1B are skipped), msg_round[i],
 * group_index[i] (NULL = 0; the acceptor group's index inside the leader's leader group), acceptor_index[i], and the
 * records offsets[i] .. offsets[i + 1] of info_slot / info_vote_round / info_value_id (offsets: n + 1 int64, FPX_NOOP the
 * value id of a Noop).  grid_cols as in fpx_proxy_phase2b_msgs: 0 = acceptor acceptor_index (0 .. replicas_total - 1) of
 * group group_index; > 0 = the bit group_index * grid_cols + acceptor_index of the single grid group (a context with one
 * group), whose rows are the grid_cols-wide runs of bits.
 * The result is exactly the handler's, message by message:
 *   1. msg_round != round: ignored, does not count (:517-526).  msg_round > round is logger.checkLt firing: the message
 *      is skipped all the same, the status is FPX_EFATAL_PROTOCOL with the lowest such index, the others still decide.
 *   2. phase1bs(group)(acceptor) = message: a later message of an acceptor replaces the earlier one whole.
 *   3. The call decides at the first index k after which the quorum condition holds: without a grid every acceptor group
 *      holds f + 1 distinct acceptors (the context's f); with a grid the context's read-quorum predicate
 *      (fpx_read_quorum_eval) holds over the bits held.  Only messages at indices <= k are used, the last per acceptor;
 *      what follows k finds the leader in Phase 2 and is ignored.  No such k: result[FPX_P1B_COMPLETE] = 0,
 *      result[FPX_P1B_DECIDED_AT] = -1, nothing else is written and no record is read.
 *   4. max_slot = the largest info_slot of the messages used (-1 if they carry none), and at least recover_slot
 *      (phase1.recoverSlot of Mencius; -1 for MultiPaxos).  Mencius checks max_slot == -1 || max_slot % num_leader_groups
 *      == leader_group: a violation is FPX_EFATAL_PROTOCOL (fpx_error_detail: index -1, the slot) and nothing is written.
 *   5. Output slots: nextClassicRound(leader_group, chosen_watermark - 1) .. max_slot in steps of num_leader_groups
 *      (MultiPaxos, one leader group: chosen_watermark .. max_slot).  Records below the watermark enter max_slot only.
 *   6. For output slot s the messages used are those of group (s / num_leader_groups) % num_groups; with a grid, those of
 *      row s % rows -- literally what Leader.scala:552 takes -- or, with FPX_P1B_GRID_ALL_ROWS, every message held.
 *   7. safe_round[j] = the highest vote_round among their records of s (-1: none), safe_value[j] = that record's value id
 *      (FPX_NOOP: none); on equal rounds the lowest bit wins (fpx_leader_phase1b_scan's rule).  out_slot[j] = s: with the
 *      leader's round a Phase2a batch for fpx_proxy_open_dev / fpx_phase2_fused_dev.
 *   8. result: FPX_P1B_COUNT entries, FPX_P1B_MAX_SLOT, FPX_P1B_NEXT_SLOT = nextClassicRound(leader_group, max_slot)
 *      (max_slot + 1 for MultiPaxos: 0 for a log without votes, whatever the watermark), FPX_P1B_WRITTEN = min(count,
 *      cap); held_bits (num_leader_groups * num_groups x 4 words, may be NULL) names the acceptors used.
 * Checked on the device before anything is written -- FPX_EINVAL, the lowest offending message index in
 * fpx_error_detail, and (the _dev convention) the context applies nothing up to the next fpx_sync: offsets not
 * non-decreasing from 0; group_index / acceptor_index outside the geometry or grid_cols; and, in the messages the result
 * uses, a record with vote_round outside 0 .. 2^30 - 2, a negative slot, or slots not strictly ascending (an acceptor's
 * states.iteratorFrom yields them so, which is what makes info.find(_.slot == slot) unambiguous).  Messages the handler
 * ignores are not read.  FPX_EINVAL at once, nothing enqueued: NULL context or result, n < 0 or >= 2^30, cap < 0, round
 * outside 0 .. 2^30 - 2, chosen_watermark < 0, recover_slot < -1, leader_group outside the leader groups, an unknown flag,
 * grid_cols outside 0 .. 256 or > 0 on a context with several groups, missing arrays.
 * Capacity as fpx_acceptor_phase1b_info_all_dev: with count > cap the first cap entries are written and the status is
 * FPX_ECAPACITY, which aborts nothing; cap = 0 with NULL arrays is the sizing call.  A context in the "apply nothing"
 * state writes result[FPX_P1B_COMPLETE] = 0 only.
 * Seven launches, nothing read by the host in between, integer atomics only (csrc/fpx_phase1b_msgs.hpp): the result is
 * reproducible bit for bit.  The scratch (a bid table of cap x 8 bytes among it) stays with the context.
 * _dev: device pointers, enqueued on the context's stream, errors at fpx_sync.  The host form is synchronous, goes
 * through the staging driver, reports bad offsets before anything is uploaded, and writes to the caller's arrays exactly
 * what the device form would have written. */
#define FPX_P1B_GRID_ALL_ROWS 1u
enum {
  FPX_P1B_COMPLETE = 0,
  FPX_P1B_DECIDED_AT = 1,
  FPX_P1B_COUNT = 2,
  FPX_P1B_MAX_SLOT = 3,
  FPX_P1B_NEXT_SLOT = 4,
  FPX_P1B_WRITTEN = 5,
  FPX_P1B_RESULT_WORDS = 8
};
int32_t fpx_leader_phase1b_msgs_dev(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, int32_t leader_group,
        int32_t recover_slot, uint32_t flags, int32_t n, const int32_t* d_kind, const int32_t* d_msg_round,
        const int32_t* d_group_index, const int32_t* d_acceptor_index, const int64_t* d_offsets /* n + 1 */,
        const int32_t* d_info_slot, const int32_t* d_info_vote_round, const int32_t* d_info_value_id, int32_t grid_cols,
        int32_t cap, int32_t* d_out_slot, int32_t* d_safe_round, int32_t* d_safe_value,
        int64_t* d_result /* FPX_P1B_RESULT_WORDS */, uint64_t* d_held_bits /* groups x 4, or NULL */);
int32_t fpx_leader_phase1b_msgs(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, int32_t leader_group,
        int32_t recover_slot, uint32_t flags, int32_t n, const int32_t* kind, const int32_t* msg_round,
        const int32_t* group_index, const int32_t* acceptor_index, const int64_t* offsets, const int32_t* info_slot,
        const int32_t* info_vote_round, const int32_t* info_value_id, int32_t grid_cols, int32_t cap, int32_t* out_slot,
        int32_t* safe_round, int32_t* safe_value, int64_t* result, uint64_t* held_bits);

/* Acceptor.maxVotedSlot (multipaxos/Acceptor.scala:104, 208) as the read path reports it (handleMaxSlotRequest /
 * handleBatchMaxSlotRequest, :222-254), restricted to the slots [first_slot, first_slot + count) of the acceptor's group:
 * the largest of them in which the acceptor holds a vote, -1 if there is none.  With first_slot = 0 and count = num_slots
 * this is the scalar fpx_read_acceptor returns; a caller that maps an unbounded log onto the context's rows (row =
 * slot % num_slots: jni/Native.scala) asks lap by lap, because the maximum over rows is not the maximum over slots once
 * the window has wrapped.  Synchronous; one strided read of the acceptor's column. */
int32_t fpx_acceptor_max_voted_in(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t first_slot, int32_t count,
                                  int32_t* max_slot);
/* Acceptor.handlePhase1a's reply (multipaxos/Acceptor.scala:163-181; mencius/Acceptor.scala:181-199): the
 * Phase1b.info of acceptor `replica` of `group` -- one Phase1bSlotInfo(slot, voteRound, voteValue) per slot >=
 * chosen_watermark in which the acceptor has voted, in ascending slot order (states.iteratorFrom).  *count = how
 * many there are; the first min(*count, cap) are written (call with cap = 0 to size the arrays).  Together with
 * fpx_acceptor_phase1a (the round movement) this is everything an acceptor-side actor needs to answer a Leader's
 * Phase1a with the Phase1b the unchanged Leader.handlePhase1b expects (multipaxos/Leader.scala:504-577). */
int32_t fpx_acceptor_phase1b_info(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t chosen_watermark,
                                  int32_t cap, int32_t* count, int32_t* slot, int32_t* vote_round,
                                  int32_t* vote_value);
/* Phase1b.info of EVERY selected acceptor in one pass; _dev convention (device pointers, enqueued on the
 * context's stream, FPX_OK once enqueued, errors at fpx_sync).  An entry is e = group * num_replicas + replica,
 * E = groups * num_replicas entries; entry e's records -- what fpx_acceptor_phase1b_info returns for it, slots
 * ascending -- are d_offsets[e] .. d_offsets[e + 1] of the three record arrays, the entries back to back in entry
 * order, d_offsets[E] the total.  An acceptor whose mask bit is clear gets an empty run (bits outside the members
 * are ignored, as fpx_acceptor_phase1a ignores them).  The vote rows are read once, coalesced, from the watermark
 * on (count, scan, scatter: csrc/fpx_phase1_info.hpp); nothing is read by the host between the passes and the
 * result is deterministic.
 * Capacity, as the device encoders of fpx_wire.h: d_totals and all E + 1 offsets are always written; with more
 * records than cap, the records at global index < cap are written and the status is FPX_ECAPACITY -- a per-call
 * code that aborts nothing.  cap = 0 with NULL record arrays is the sizing call.  FPX_EINVAL at once, nothing
 * enqueued: NULL context, negative cap, missing offsets or totals, missing record arrays with cap > 0.  A context
 * in the "apply nothing" state writes d_totals = {0, 0} and d_offsets[0] = 0 only. */
int32_t fpx_acceptor_phase1b_info_all_dev(fpx_ctx* ctx, int32_t chosen_watermark,
        const uint64_t* d_acceptor_masks /* ngroups x 4, bit convention of fpx_acceptor_phase1a's target_mask; NULL = all */,
        int64_t cap, int64_t* d_offsets /* E + 1 */, int32_t* d_slot, int32_t* d_vote_round, int32_t* d_vote_value,
        int64_t* d_totals /* [0] = records needed, [1] = records written */);
/* host arrays, synchronous, through the staging driver the other host-pointer entry points use; *count = records
 * needed.  The records are staged in three device buffers of cap x 4 bytes each, which the context keeps (like every
 * staging buffer) until fpx_destroy: 3 x 512 MiB after one leader change of 2^20 slots x 256 acceptors. */
int32_t fpx_acceptor_phase1b_info_all(fpx_ctx* ctx, int32_t chosen_watermark, const uint64_t* acceptor_masks,
        int64_t cap, int64_t* offsets, int32_t* slot, int32_t* vote_round, int32_t* vote_value, int64_t* count);
/* A Leader's Phase1a broadcast at every acceptor it addresses, one call: fpx_acceptor_phase1a for each group with
 * a non-empty mask (in group order; target_masks NULL = every acceptor of every group), then the info of exactly
 * the acceptors that promised.  With FPX_ECAPACITY the promises were applied.  The round a Nack carries stays
 * with fpx_read_acceptor / the per-acceptor call. */
int32_t fpx_acceptor_phase1(fpx_ctx* ctx, int32_t round, int32_t chosen_watermark, const uint64_t* target_masks,
        uint64_t* promised_bits /* ngroups x 4 */, uint64_t* nack_bits /* ngroups x 4 */,
        int64_t cap, int64_t* offsets, int32_t* slot, int32_t* vote_round, int32_t* vote_value, int64_t* count);

/* ---- state readback (parity) ------------------------------------------------------------------- */
/* acceptor `replica` of `group`: its round (FPX_BALLOT_ACCEPTOR; -1 in PER_SLOT mode),
 * maxVotedSlot, and for every slot s in [0, S): vote_round[s] / vote_value[s] (-1 / -1 when the
 * acceptor has no vote in s or s belongs to another group) and, in PER_SLOT mode, ballot[s].
 * Array arguments may be NULL. */
int32_t fpx_read_acceptor(fpx_ctx* ctx, int32_t group, int32_t replica, int32_t* promised,
                          int32_t* max_voted_slot, int32_t* vote_round, int32_t* vote_value,
                          int32_t* ballot);
/* whole-array readback, slot-major [S][R] int32 (may be NULL each).  FPX_BALLOT_PER_SLOT with more than 128 acceptors
 * per group keeps the votes of a row in which the whole group voted as one (round, value) record instead of 2 x R cells
 * (fpx_vote_summary_audit); a readback of either vote array first writes every such record into its row's cells, so a
 * read-only caller still costs those rows their 2 KiB each and their compact form -- fpx_read_acceptor,
 * fpx_state_digest and the Phase1b entry points answer from the records and leave them. */
int32_t fpx_read_state(fpx_ctx* ctx, int32_t* vote_round, int32_t* vote_value, int32_t* ballot);
/* per-acceptor scalars, [num_leader_groups * num_groups][R] */
int32_t fpx_read_scalars(fpx_ctx* ctx, int32_t* promised, int32_t* max_voted_slot);
/* proxy-leader tallies of one slot: up to tally_ways entries; state 0 = Pending, 1 = Done */
int32_t fpx_read_tally(fpx_ctx* ctx, int32_t slot, int32_t* num_entries, int32_t* rounds,
                       int32_t* states, int32_t* values, uint64_t* vote_bits /* ways x 4 */);

/* ---- multi-GPU: one context per GPU, one RCCL communicator over them ----------
 *
 * The Phase-2 path shards two ways.
 * (1) By acceptor group -- no exchange step: slot -> group is fixed (multipaxos/ProxyLeader.scala:190,
 *     mencius/ProxyLeader.scala:231-234) and groups never interact in Phase 2, so rank r simply owns the
 *     groups g with g % world == r and runs the single-GPU entry points on its own slots.  Only Chosen
 *     records leave a GPU; fpx_comm_allgather_chosen_dev hands every rank all of them when a device-side
 *     replica log is kept on each GPU (13 B per slot per rank over xGMI).
 * (2) By the acceptor axis of ONE big group (flexible mode: "the log is not partitioned",
 *     multipaxos/Config.scala:16-21) -- one exchange step, replacing the fan-in of every acceptor's Phase2b
 *     to one proxy leader (multipaxos/ProxyLeader.scala:217-258): the context of rank r is created with
 *     replica_base = r * R / world, num_replicas = R / world, replicas_total = R;
 *     fpx_phase2_replica_sharded_dev runs K1 on its acceptor columns for all n slots (partial 256-bit vote
 *     bitmaps with bits only in its own range), ONE ncclReduceScatter(ncclSum, ncclUint64) of the 4 n words
 *     (disjoint bit ranges: sum == OR and never carries) gives rank r the full bitmaps of ITS n / world
 *     slots, and the proxy-leader open + tally (K2) runs on that slice.  xGMI traffic per GPU and call:
 *     a ring reduce-scatter sends and receives (world - 1) / world x 32 B x n (28 MiB for n = 2^20 at
 *     world = 8, ~0.2 ms at one 153 GB/s link); an all-reduce would move twice that and make every GPU tally
 *     all n slots.
 * RCCL is loaded at run time (an RCCL already in the process -- PyTorch's -- is reused; else librccl.so.1 /
 * $FPX_RCCL_LIB): single-GPU callers never need it.  The id comes from fpx_comm_unique_id on one rank and
 * reaches the others out of band (the JVM actors' own transport, MPI, a torch.distributed broadcast ...). */
#define FPX_COMM_ID_BYTES 128
int32_t fpx_comm_unique_id(uint8_t id[FPX_COMM_ID_BYTES]);
/* collective: every rank calls it with the same id and world, its own rank; binds the communicator to ctx */
int32_t fpx_comm_create(fpx_ctx* ctx, const uint8_t id[FPX_COMM_ID_BYTES], int32_t rank, int32_t world);
int32_t fpx_comm_destroy(fpx_ctx* ctx);
int32_t fpx_comm_info(fpx_ctx* ctx, int32_t* rank, int32_t* world); /* (0, 1) without a communicator */
int32_t fpx_last_rccl_error(fpx_ctx* ctx);
/* (2) above.  n must be a multiple of world; all ranks pass the same n messages (device pointers,
 * asynchronous on the context's stream, run contract as for the other _dev calls).  d_target_mask: n x 4
 * words over the WHOLE group (bit j = acceptor j of replicas_total) or NULL.  Outputs cover this rank's
 * slice of the batch, messages [rank * n / world, (rank + 1) * n / world): d_chosen / d_chosen_round /
 * d_chosen_value have n / world entries (as fpx_proxy_phase2b_dev); d_nack_round (n entries or NULL) is the
 * largest round Nacked by ANY rank's acceptors (ncclAllReduce(ncclMax) of the ranks' own, in place: the same n
 * values on every rank).  Without a communicator (world 1) it is K1 + open + K2. */
int32_t fpx_phase2_replica_sharded_dev(fpx_ctx* ctx, int32_t n, const int32_t* d_slot, const int32_t* d_round,
                                       const int32_t* d_value_id, const uint64_t* d_target_mask,
                                       uint8_t* d_chosen, int32_t* d_chosen_round, int32_t* d_chosen_value,
                                       int32_t* d_nack_round);
/* (1) above: all-gather of the Chosen records of n_local messages per rank; the d_all_* arrays have
 * world x n_local entries, rank-major.  Any of the three pairs may be NULL. */
int32_t fpx_comm_allgather_chosen_dev(fpx_ctx* ctx, int32_t n_local, const uint8_t* d_chosen,
                                      const int32_t* d_chosen_round, const int32_t* d_chosen_value,
                                      uint8_t* d_all_chosen, int32_t* d_all_round, int32_t* d_all_value);
/* with fpx_profile_enable: number and summed duration of the collectives since the last read (HIP events
 * on the context's stream around each RCCL call) */
int32_t fpx_profile_read_collective(fpx_ctx* ctx, int32_t* launches, double* total_ms);

/* Whole-state digests for parity checks at sizes where a readback is gigabytes: out[0..6] =
 * vote_round cells, vote_value cells, ballot cells (0 in FPX_BALLOT_ACCEPTOR mode), acceptors' rounds,
 * acceptors' maxVotedSlot, the proxy leader's single-slot tallies, the replica's log (+ executedWatermark,
 * numChosen), the proxy leader's noop-range tallies.  Each is an order-independent wrapping sum of a 64-bit hash per element (per cell
 * (slot, acceptor): splitmix64-finalise((slot * R + acceptor) * 0x9E3779B97F4A7C15 + (uint32)value + 1)), so
 * equal digests <=> equal state up to 2^-64.  Waits for the stream. */
int32_t fpx_state_digest(fpx_ctx* ctx, uint64_t out[8]);

/* FPX_BALLOT_PER_SLOT: audit of the per-row ballot summaries (one round per row that every stored ballot cell of
 * the row holds, or "mixed"), a test hook.  out[0] = rows summarised as uniform, out[1] = rows marked mixed,
 * out[2] = violations: uniform rows with a stored cell that differs from the summary (must be 0).  Outstanding
 * lazy Phase1a promises are left as they are (the summaries describe the stored cells).  Groups of at most 128
 * acceptors keep no summaries: every row counts as mixed.  FPX_EINVAL in FPX_BALLOT_ACCEPTOR mode.  Waits for the
 * stream. */
int32_t fpx_ballot_summary_audit(fpx_ctx* ctx, int64_t out[3]);

/* The states of the vote rows, a test hook.  out[0] = fresh rows (no vote, every cell -1), out[1] = rows whose cells are
 * authoritative, out[2] = compact rows: every acceptor of the row's group holds the row's (round, value) record and the
 * stored cells are unspecified.  Records are kept where the ballot summaries are (FPX_BALLOT_PER_SLOT, more than 128
 * acceptors per group); elsewhere out[2] is 0.  out[0] + out[1] + out[2] = num_slots.  A row goes compact when a batch
 * without target masks has the whole group vote in it; it becomes cells again when a dense batch delivers a message to
 * it that not the whole group accepts, and when a batch WITH target masks names its slot (delivered or not).  Waits for
 * the stream. */
int32_t fpx_vote_summary_audit(fpx_ctx* ctx, int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* FPX_H */
