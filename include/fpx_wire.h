/*
 * fpx_wire.h -- wire adapter of libfpx: the reference's protobuf messages of the
 * Phase-2 path <-> the struct-of-arrays batches of include/fpx.h.  Plain C ABI.  The functions that take no context are
 * host code (no GPU involved); the _dev entry points decode a tick and encode its replies ON THE GPU, and
 * fpx_wire_phase2_tick runs a whole proxy-leader tick bytes to bytes.
 *
 * The reference's actors exchange ScalaPB messages serialised with `toByteArray` / parsed with `parseFrom`
 * (shared/src/main/scala/frankenpaxos/ProtoSerializer.scala:8-9) and wrapped in one `...Inbound` oneof per actor:
 *
 *   ProxyLeaderInbound { oneof request { Phase2a phase2a = 1; Phase2b phase2b = 2; } }      MultiPaxos.proto:541-549
 *   AcceptorInbound    { oneof request { Phase1a phase1a = 1; Phase2a phase2a = 2; ... } }   MultiPaxos.proto:551-561
 *   ReplicaInbound     { oneof request { Chosen chosen = 1; ... } }                          MultiPaxos.proto:563-575
 *   LeaderInbound      { oneof request { ...; Nack nack = 6; ... } }                         MultiPaxos.proto:525-539
 *   Phase1a { required int32 round = 1; required int32 chosen_watermark = 2; }               MultiPaxos.proto:238-253
 *   Phase2a { required int32 slot = 1; required int32 round = 2;
 *             required CommandBatchOrNoop command_batch_or_noop = 3; }                       MultiPaxos.proto:273-281
 *   Phase2b { required int32 group_index = 1; required int32 acceptor_index = 2;
 *             required int32 slot = 3; required int32 round = 4; }                           MultiPaxos.proto:283-291
 *   Chosen  { required int32 slot = 1; required CommandBatchOrNoop command_batch_or_noop = 2; }   MultiPaxos.proto:293-299
 *   Nack    { required int32 round = 1; }                                                    MultiPaxos.proto:455-460
 *   CommandBatchOrNoop { oneof value { CommandBatch command_batch = 1; Noop noop = 2; } }    MultiPaxos.proto:213-221
 *
 * A transport wrapper collects the byte arrays one event-loop tick delivers to an actor into ONE
 * buffer plus n + 1 offsets, decodes them here into the SoA arrays of a batch, calls the fpx_* entry point, and
 * encodes the replies (Phase2b / Chosen / Nack) back.  The command payload (CommandBatchOrNoop) never travels to
 * the GPU: the decoder reports where its bytes are, the caller keeps them under the value_id it hands to libfpx
 * (FPX_NOOP for Noop) and splices them back into Chosen when that value_id comes out of the tally.
 *
 * Encoding is canonical protobuf (fields in number order, required fields always present, int32 as varint with
 * negative values sign-extended to 10 bytes), i.e. byte-identical to ScalaPB's toByteArray for these messages;
 * the decoder accepts any valid encoding (fields in any order, unknown fields skipped).
 */
#ifndef FPX_WIRE_H
#define FPX_WIRE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FPX_WIRE_OTHER = 0,   /* a well-formed message of a kind this path does not handle: left to the JVM actor */
  FPX_WIRE_PHASE2A = 1,
  FPX_WIRE_PHASE2B = 2,
  FPX_WIRE_PHASE1A = 3,
  FPX_WIRE_CHOSEN = 4,
  FPX_WIRE_NACK = 5,
  FPX_WIRE_PHASE1B = 9,
  /* the acceptor's read path (multipaxos/Acceptor.scala:222-254) */
  FPX_WIRE_MAX_SLOT_REQUEST = 10,
  FPX_WIRE_BATCH_MAX_SLOT_REQUEST = 11,
  /* the replica's read path (multipaxos/Replica.scala:455-529, 629-690): ReplicaInbound fields 2 - 7.  A ...BATCH is ONE
   * message: its commands share one slot and one fate */
  FPX_WIRE_READ_REQUEST = 12,
  FPX_WIRE_SEQUENTIAL_READ_REQUEST = 13,
  FPX_WIRE_EVENTUAL_READ_REQUEST = 14,
  FPX_WIRE_READ_REQUEST_BATCH = 24,
  FPX_WIRE_SEQUENTIAL_READ_REQUEST_BATCH = 25,
  FPX_WIRE_EVENTUAL_READ_REQUEST_BATCH = 26,
  /* mencius/Mencius.proto */
  FPX_WIRE_PHASE2A_NOOP_RANGE = 6,
  FPX_WIRE_PHASE2B_NOOP_RANGE = 7,
  FPX_WIRE_CHOSEN_NOOP_RANGE = 8,
  /* epaxos/EPaxos.proto: the members of ReplicaInbound, by their field number + 14 */
  FPX_WIRE_EPX_PRE_ACCEPT = 16,
  FPX_WIRE_EPX_PRE_ACCEPT_OK = 17,
  FPX_WIRE_EPX_ACCEPT = 18,
  FPX_WIRE_EPX_ACCEPT_OK = 19,
  FPX_WIRE_EPX_COMMIT = 20,
  FPX_WIRE_EPX_PREPARE = 21,
  FPX_WIRE_EPX_PREPARE_OK = 22,
  FPX_WIRE_EPX_NACK = 23
  /* 24 - 26: the replica's read batches, above */
};

/* Decodes n ProxyLeaderInbound messages: message i is buf[offsets[i] .. offsets[i + 1]); buf_len = the bytes buf
 * holds: the n + 1 offsets must be non-negative, non-decreasing and at most buf_len, which is checked for ALL of them
 * before anything is parsed (FPX_EINVAL, *bad_index = the first offender).  Per message:
 * kind[i] (PHASE2A / PHASE2B / OTHER); Phase2a: slot, round, is_noop, and the location of the serialised
 * CommandBatchOrNoop inside buf (value_off, value_len); Phase2b: group_index, acceptor_index, slot, round.
 * Fields that do not apply are set to -1.  Returns FPX_OK, or FPX_EINVAL at the first malformed message (truncated
 * varint, length past the end, missing required field); *bad_index (may be NULL) tells which. */
int32_t fpx_wire_decode_proxy_leader_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n, int32_t* kind,
                                             int32_t* slot, int32_t* round, int32_t* is_noop, int64_t* value_off,
                                             int32_t* value_len, int32_t* group_index, int32_t* acceptor_index,
                                             int32_t* bad_index);
/* Decodes n AcceptorInbound messages: kind PHASE1A (round, chosen_watermark) / PHASE2A (slot, round, value) /
 * MAX_SLOT_REQUEST (value_off, value_len = where the serialised CommandId lies: the reply returns it unchanged) /
 * BATCH_MAX_SLOT_REQUEST (slot = read_batcher_index, round = read_batcher_id) / OTHER. */
int32_t fpx_wire_decode_acceptor_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n, int32_t* kind,
                                         int32_t* slot, int32_t* round, int32_t* is_noop, int64_t* value_off,
                                         int32_t* value_len, int32_t* chosen_watermark, int32_t* bad_index);
/* Decodes n ReplicaInbound messages: kind CHOSEN (slot, value) / OTHER. */
int32_t fpx_wire_decode_replica_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n, int32_t* kind,
                                        int32_t* slot, int32_t* is_noop, int64_t* value_off, int32_t* value_len,
                                        int32_t* bad_index);

/* Decodes n ReplicaInbound messages WITH the replica's read path (fields 1 - 7, MultiPaxos.proto:351-396, 566-575):
 * kind CHOSEN (slot, is_noop, value_off / value_len as above; count -1) / READ_REQUEST, SEQUENTIAL_READ_REQUEST (slot =
 * the request's slot; value_off / value_len = where the serialised Command lies; count 1) / EVENTUAL_READ_REQUEST (slot
 * -1; the Command; count 1) / READ_REQUEST_BATCH, SEQUENTIAL_READ_REQUEST_BATCH, EVENTUAL_READ_REQUEST_BATCH (slot, -1
 * for the eventual one; value_off / value_len = the whole inner message; count = its number of commands, 0 included) /
 * OTHER.  Every Command is checked for its required fields (command_id with its three, command).  kind and slot are
 * required, the other arrays may be NULL; the arrays feed fpx_replica_inbox.  Malformed input as in the other decoders.
 * Host only. */
int32_t fpx_wire_decode_replica_inbound_reads(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n,
                                              int32_t* kind, int32_t* slot, int32_t* is_noop, int64_t* value_off,
                                              int32_t* value_len, int32_t* count, int32_t* bad_index);

/* The two decoders above ON THE DEVICE: the tick's bytes and its n + 1 offsets are device pointers (or page-locked host
 * memory the GPU can read), the outputs are device arrays of n elements, and the work is enqueued on the context's
 * stream like every _dev entry point of include/fpx.h -- a tick goes  copy -> decode -> fpx_phase2_fused_dev /
 * fpx_acceptor_phase2a_dev  without the host parsing a byte.  One thread per message runs the SAME parser the host
 * decoders run (csrc/fpx_wire_parse.hpp is compiled for both sides), so the fields are identical: kind, slot, round,
 * is_noop, value_off, value_len and group_index / acceptor_index (resp. chosen_watermark), -1 where a field does not
 * apply; d_kind, d_slot and d_round are required, the others may be NULL.  d_value_id (may be NULL): value_id_base + i
 * for a Phase2a, -1 otherwise -- the id under which the caller files message i's command bytes (value_off, value_len)
 * and which the Phase-2 kernels carry through to Chosen.
 * Errors follow the _dev convention: the call returns FPX_OK once enqueued; a bad offset or a malformed message makes
 * the context's status FPX_EINVAL (fpx_sync; fpx_error_detail's index = the first bad offset, else the first
 * malformed message, as *bad_index above) and every later _dev call up to that fpx_sync applies nothing, so a
 * half-decoded tick never reaches the acceptors.  The outputs of a failed decode are unspecified.  n < 2^30. */
struct fpx_ctx;
int32_t fpx_wire_decode_proxy_leader_inbound_dev(struct fpx_ctx* ctx, const uint8_t* d_buf, int64_t buf_len,
                                                 const int64_t* d_offsets, int32_t n, int32_t* d_kind, int32_t* d_slot,
                                                 int32_t* d_round, int32_t* d_is_noop, int64_t* d_value_off,
                                                 int32_t* d_value_len, int32_t* d_group_index,
                                                 int32_t* d_acceptor_index, int32_t value_id_base, int32_t* d_value_id);
int32_t fpx_wire_decode_acceptor_inbound_dev(struct fpx_ctx* ctx, const uint8_t* d_buf, int64_t buf_len,
                                             const int64_t* d_offsets, int32_t n, int32_t* d_kind, int32_t* d_slot,
                                             int32_t* d_round, int32_t* d_is_noop, int64_t* d_value_off,
                                             int32_t* d_value_len, int32_t* d_chosen_watermark, int32_t value_id_base,
                                             int32_t* d_value_id);

/* ---- the encoders ON THE DEVICE ----------------------------------------------------------------------------------
 * The replies of a tick as wire bytes without the records coming down first: what fpx_phase2_fused_dev /
 * fpx_acceptor_phase2a_dev left in HBM (Chosen flags, vote bits, Nack rounds) and what the device decoder left there
 * (slot, is_noop, value_off, value_len, and the tick's bytes themselves) go in, the serialised messages come out back to
 * back.  _dev convention: device pointers, enqueued on the context's stream, FPX_OK once enqueued, errors at fpx_sync.
 * Shared contract:
 *   bytes    d_out is, byte for byte, the concatenation of what the host encoder returns for the same records in the
 *            same order (one emitter source, csrc/fpx_wire_emit.hpp, compiled for both sides).
 *   offsets  d_out_offsets[k] = start of message k, d_out_offsets[count] = the total.
 *   totals   d_totals[0] = count, d_totals[1] = the bytes needed: ALWAYS written, valid after fpx_sync.
 *   FPX_ECAPACITY  the bytes needed exceed cap, or count exceeds max_msgs: no byte of d_out and no entry of
 *            d_out_offsets beyond [0] (= 0) is written; d_totals says what to allocate.  A PER-CALL code, not an abort:
 *            later _dev calls on the context apply as usual (the votes are applied already, the caller only encodes
 *            again).  Like every device status it is sticky up to the next fpx_sync, which returns and clears it.
 *   FPX_EINVAL     (Chosen) an emitted, non-Noop record whose value_off / value_len leave [0, values_len]:
 *            fpx_error_detail's index names the first one, nothing is written beyond d_totals and d_out_offsets[0];
 *            also a per-call code.  A negative value_len counts as 0, as in the host encoder.
 *   empty    n == 0 or nothing to emit: count 0, d_out_offsets[0] = 0, FPX_OK.
 *   aborted run  if the context is in the "apply nothing" state (a malformed tick, a run-contract violation) nothing
 *            is encoded either: d_totals and d_out_offsets[0] are written, d_out is not.
 *   graphs   no host wait inside, so a call can be captured into a HIP graph -- once the context's scratch is sized:
 *            the first call with a larger n than any before allocates (8 bytes per 128 records), so run one call with
 *            the largest n outside the capture.
 * NULL context, n < 0 or n >= 2^30, negative cap / max_msgs, a missing required array: FPX_EINVAL at once, nothing is
 * enqueued.  d_out may be NULL when cap == 0 (a sizing call: FPX_ECAPACITY and d_totals).
 * Deviations from the issue's proposal: none in the signatures; the scratch note under "graphs" above. */
enum { FPX_WIRE_MULTIPAXOS = 0, FPX_WIRE_MENCIUS = 1 }; /* dialect: which .proto's layout */

/* ReplicaInbound{Chosen(slot, command_batch_or_noop)} for every record i with d_emit[i] != 0 (NULL = all), in index
 * order.  Value of record i: d_values[d_value_off[i] .. + d_value_len[i]), or Noop where d_is_noop[i] != 0 (NULL = none):
 * exactly fpx_wire_encode_replica_chosen's choice.  The two dialects share this message (same shape, same field
 * numbers).  d_out_offsets has n + 1 entries, d_totals 2. */
int32_t fpx_wire_encode_replica_chosen_dev(struct fpx_ctx* ctx, int32_t n, const uint8_t* d_emit, const int32_t* d_slot,
                                           const int32_t* d_is_noop, const uint8_t* d_values, int64_t values_len,
                                           const int64_t* d_value_off, const int32_t* d_value_len, uint8_t* d_out,
                                           int64_t cap, int64_t* d_out_offsets, int64_t* d_totals);
/* fpx_wire_encode_phase2b_batch on the device: one ProxyLeaderInbound{Phase2b} per set bit of d_vote_bits (n x 4
 * words), message-major, bits ascending; bit -> (group_index, acceptor_index) as the host encoder maps it
 * (d_group_of_slot may be NULL: group 0).  dialect FPX_WIRE_MENCIUS: Mencius.proto's Phase2b (acceptor_index, slot,
 * round; wrapper field 4).  d_out_offsets has max_msgs + 1 entries. */
int32_t fpx_wire_encode_phase2b_batch_dev(struct fpx_ctx* ctx, int32_t dialect, int32_t n, const int32_t* d_slot,
                                          const int32_t* d_round, const uint64_t* d_vote_bits,
                                          const int32_t* d_group_of_slot, int32_t grid_cols, uint8_t* d_out, int64_t cap,
                                          int64_t* d_out_offsets, int64_t max_msgs, int64_t* d_totals);
/* LeaderInbound{Nack(round)} for every record with d_nack_round[i] >= 0 (what K1 / K3 report), in index order; wrapper
 * field 6 (MultiPaxos) / 7 (Mencius). */
int32_t fpx_wire_encode_leader_nack_dev(struct fpx_ctx* ctx, int32_t dialect, int32_t n, const int32_t* d_nack_round,
                                        uint8_t* d_out, int64_t cap, int64_t* d_out_offsets, int64_t max_msgs,
                                        int64_t* d_totals);

/* One proxy-leader tick, bytes to bytes, on PAGE-LOCKED buffers (fpx_host_alloc; FPX_EINVAL for anything else): n
 * serialised ProxyLeaderInbound{Phase2a} messages (in, in_len, in_offsets[n + 1]) -> copy up ->
 * fpx_wire_decode_proxy_leader_inbound_dev -> fpx_phase2_fused_dev (target_mask NULL, value_id = the message's index) ->
 * fpx_wire_encode_replica_chosen_dev -> copy down: the ReplicaInbound{Chosen} messages of the tick in message order
 * (out, out_offsets[count + 1], *out_count), each carrying the value bytes of the Phase2a it answers, and the Nack
 * rounds (nack_round[n], may be NULL; -1 = none).  Synchronous.
 * Every message must be a Phase2a: anything else, a malformed message or a bad offset is FPX_EINVAL with *bad_index
 * (may be NULL), and the tick must be one device run (FPX_EORDER, *bad_index: as fpx_phase2_fused_submit); in both
 * cases NOTHING is applied.
 * Sizing out: a Chosen is never longer than the Phase2a it answers -- it drops the round field (at least two bytes),
 * its slot is the same non-negative int32 in its shortest form, its value is the same bytes (or the two bytes of a Noop
 * where the Phase2a's value was at least those two), and the two length prefixes can only shrink -- so out_cap >= in_len
 * (with out_offsets of n + 1 entries) makes FPX_ECAPACITY unreachable.  A caller who passes less may get FPX_ECAPACITY:
 * the tick WAS applied, out holds nothing, *bytes_needed (may be NULL; set on FPX_OK too) is what it would have taken.
 * The copy down moves out_cap bytes (what lies in out behind the messages, up to out_cap, is unspecified): do not pass
 * much more than in_len. */
int32_t fpx_wire_phase2_tick(struct fpx_ctx* ctx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets, int32_t n,
                             uint8_t* out, int64_t out_cap, int64_t* out_offsets, int64_t* out_count,
                             int32_t* nack_round, int64_t* bytes_needed, int32_t* bad_index);

/* One tick of a proxy leader among REMOTE acceptors, bytes to records, on PAGE-LOCKED buffers (fpx_host_alloc;
 * FPX_EINVAL for anything else): n serialised ProxyLeaderInbound messages (in, in_len, in_offsets[n + 1]) -> copy up ->
 * fpx_wire_decode_proxy_leader_inbound_dev -> fpx_proxy_phase2b_msgs_dev (include/fpx.h) -> the newly chosen records
 * compacted on the device in message order -> copy down of the count and the records only.  Synchronous.
 * Record k = (out_slot[k], out_round[k], out_value_id[k]): the k-th (slot, round) that reached its quorum in this tick
 * and the value id given to fpx_proxy_open.  The outputs are records, not Chosen bytes: the value bytes belong to the
 * Phase2a of an earlier tick and stay with the caller under their value id.  Phase2a messages (and any other kind) in
 * the tick are skipped: the caller opens and forwards them.
 * A malformed message or a bad offset is FPX_EINVAL with *bad_index (may be NULL) and NOTHING is applied, as is a Phase2b
 * that fpx_proxy_phase2b_msgs refuses.  out_cap (records) too small is FPX_ECAPACITY: the tick WAS applied, *out_count
 * holds the count needed and the first out_cap records are written.  FPX_EFATAL_UNKNOWN_SLOTROUND: per message, the
 * others were applied and their records are out (compare *out_count with out_cap: this status outranks FPX_ECAPACITY).
 * The copy down moves out_cap records (what lies in the arrays behind the *out_count records, up to out_cap, is
 * unspecified): size out_cap by the slots that can complete in a tick, not by n. */
int32_t fpx_wire_phase2b_tick(struct fpx_ctx* ctx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets, int32_t n,
                              int32_t grid_cols, int32_t* out_slot, int32_t* out_round, int32_t* out_value_id,
                              int32_t out_cap, int32_t* out_count, int32_t* bad_index);

/* Folds decoded Phase2b messages into the rows fpx_proxy_phase2b takes: one row per distinct (slot, round), in
 * order of first appearance, with the acceptors that answered as a 256-bit set.  Bit of a message =
 * acceptor_index when grid_cols == 0 (non-flexible: the acceptor group follows from the slot,
 * multipaxos/ProxyLeader.scala:190) or group_index * grid_cols + acceptor_index for a grid (group_index = row,
 * Grid.scala).  Messages whose kind is not PHASE2B are skipped.  row_* have room for n rows; *num_rows is set.
 * FPX_EINVAL if a bit falls outside 0..255. */
int32_t fpx_wire_phase2b_rows(int32_t n, const int32_t* kind, const int32_t* group_index,
                              const int32_t* acceptor_index, const int32_t* slot, const int32_t* round,
                              int32_t grid_cols, int32_t* num_rows, int32_t* row_slot, int32_t* row_round,
                              uint64_t* row_bits /* n x 4 */);

/* Encoders.  Each writes ONE wrapped message to out and returns its length, or the negated length needed when
 * cap is too small (nothing written).  value / value_len: the serialised CommandBatchOrNoop as the decoder
 * located it; is_noop != 0 encodes CommandBatchOrNoop{noop} and ignores value. */
int64_t fpx_wire_encode_proxy_leader_phase2a(uint8_t* out, int64_t cap, int32_t slot, int32_t round,
                                             const uint8_t* value, int32_t value_len, int32_t is_noop);
int64_t fpx_wire_encode_acceptor_phase2a(uint8_t* out, int64_t cap, int32_t slot, int32_t round,
                                         const uint8_t* value, int32_t value_len, int32_t is_noop);
int64_t fpx_wire_encode_acceptor_phase1a(uint8_t* out, int64_t cap, int32_t round, int32_t chosen_watermark);
int64_t fpx_wire_encode_proxy_leader_phase2b(uint8_t* out, int64_t cap, int32_t group_index, int32_t acceptor_index,
                                             int32_t slot, int32_t round);
int64_t fpx_wire_encode_replica_chosen(uint8_t* out, int64_t cap, int32_t slot, const uint8_t* value,
                                       int32_t value_len, int32_t is_noop);
int64_t fpx_wire_encode_leader_nack(uint8_t* out, int64_t cap, int32_t round);
/* The acceptor's answers on the read path (multipaxos/Acceptor.scala:222-254):
 *   ClientInbound { oneof request { ...; MaxSlotReply max_slot_reply = 4; ... } }                 MultiPaxos.proto:489-499
 *   MaxSlotReply { CommandId command_id = 1; group_index = 2; acceptor_index = 3; slot = 4 }      :323-331
 *   ReadBatcherInbound { oneof request { ...; BatchMaxSlotReply batch_max_slot_reply = 4; } }     :513-523
 *   BatchMaxSlotReply { read_batcher_index = 1; read_batcher_id = 2; acceptor_index = 3; slot = 4 }   :341-349
 * command_id / command_id_len: the serialised CommandId as the decoder located it.  slot = Acceptor.maxVotedSlot (-1 before
 * the first vote: a negative int32 is a ten-byte varint). */
int64_t fpx_wire_encode_client_max_slot_reply(uint8_t* out, int64_t cap, const uint8_t* command_id, int32_t command_id_len,
                                              int32_t group_index, int32_t acceptor_index, int32_t slot);
int64_t fpx_wire_encode_read_batcher_batch_max_slot_reply(uint8_t* out, int64_t cap, int32_t read_batcher_index,
                                                          int32_t read_batcher_id, int32_t acceptor_index, int32_t slot);

/* The acceptor's answer to a Phase1a (multipaxos/Acceptor.scala:163-181), as the Leader parses it:
 *   LeaderInbound { oneof request { Phase1b phase1b = 1; ...; Nack nack = 6; ... } }          MultiPaxos.proto:525-539
 *   Phase1b { required int32 group_index = 1; required int32 acceptor_index = 2; required int32 round = 3;
 *             repeated Phase1bSlotInfo info = 4; }                                            MultiPaxos.proto:263-271
 *   Phase1bSlotInfo { required int32 slot = 1; required int32 vote_round = 2;
 *                     required CommandBatchOrNoop vote_value = 3; }                           MultiPaxos.proto:254-261
 * Entry j's CommandBatchOrNoop body is values[value_off[j] .. + value_len[j]) (the JVM-side bytes kept under the
 * value id fpx_acceptor_phase1b_info returned), or Noop where is_noop[j] != 0 (is_noop may be NULL: none is). */
int64_t fpx_wire_encode_leader_phase1b(uint8_t* out, int64_t cap, int32_t group_index, int32_t acceptor_index,
                                       int32_t round, int32_t n_info, const int32_t* slot, const int32_t* vote_round,
                                       const uint8_t* values, const int64_t* value_off, const int32_t* value_len,
                                       const uint8_t* is_noop);
/* Decodes n LeaderInbound messages: kind PHASE1B (round, group_index, acceptor_index, info) / NACK (round) / OTHER.
 * The Phase1bSlotInfo entries of all messages go, in order, into the info_* arrays (capacity info_cap entries;
 * FPX_EINVAL if there are more): message i owns entries info_first[i] .. info_first[i] + info_count[i]. */
int32_t fpx_wire_decode_leader_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n,
                                       int32_t* kind, int32_t* round, int32_t* group_index, int32_t* acceptor_index,
                                       int32_t* info_first, int32_t* info_count, int32_t info_cap, int32_t* info_total,
                                       int32_t* info_slot, int32_t* info_vote_round, int32_t* info_is_noop,
                                       int64_t* info_value_off, int32_t* info_value_len, int32_t* bad_index);

/* The replies of one K1 batch as wire bytes: for message i every acceptor in vote_bits[i] answers
 * ProxyLeaderInbound{Phase2b(group_index, acceptor_index, slot[i], round[i])} (Acceptor.scala:211-219).  The bit
 * -> (group_index, acceptor_index) map is the inverse of fpx_wire_phase2b_rows (group_of_slot[i] supplies the
 * group when grid_cols == 0; may be NULL for group 0).  Messages are written back to back into out;
 * out_offsets gets count + 1 entries (capacity max_msgs + 1).  Returns the number of messages, or -1 if out or
 * out_offsets is too small. */
int64_t fpx_wire_encode_phase2b_batch(int32_t n, const int32_t* slot, const int32_t* round,
                                      const uint64_t* vote_bits, const int32_t* group_of_slot, int32_t grid_cols,
                                      uint8_t* out, int64_t cap, int64_t* out_offsets, int64_t max_msgs);

/* ---- Mencius (shared/src/main/scala/frankenpaxos/mencius/Mencius.proto) ---------------------------------------
 *
 *   ProxyLeaderInbound { oneof request { HighWatermark high_watermark = 1; Phase2a phase2a = 2;
 *                        Phase2aNoopRange phase2a_noop_range = 3; Phase2b phase2b = 4;
 *                        Phase2bNoopRange phase2b_noop_range = 5; } }                         Mencius.proto:339-350
 *   AcceptorInbound    { oneof request { Phase1a phase1a = 1; Phase2a phase2a = 2;
 *                        Phase2aNoopRange phase2a_noop_range = 3; } }                         Mencius.proto:352-361
 *   ReplicaInbound     { oneof request { Chosen chosen = 1; ChosenNoopRange chosen_noop_range = 2; } }   :363-371
 *   LeaderInbound      { oneof request { ...; Nack nack = 7; ... } }                          Mencius.proto:322-337
 *   Phase2a          { slot = 1; round = 2; command_batch_or_noop = 3; }                      Mencius.proto:151-158
 *   Phase2aNoopRange { slot_start_inclusive = 1; slot_end_exclusive = 2; round = 3; }         Mencius.proto:160-168
 *   Phase2b          { acceptor_index = 1; slot = 2; round = 3; }   (no group: it follows from the slot)  :169-176
 *   Phase2bNoopRange { acceptor_group_index = 1; acceptor_index = 2; slot_start_inclusive = 3;
 *                      slot_end_exclusive = 4; round = 5; }                                   Mencius.proto:178-187
 *   Chosen           { slot = 1; command_batch_or_noop = 2; }                                 Mencius.proto:189-195
 *   ChosenNoopRange  { slot_start_inclusive = 1; slot_end_exclusive = 2; }                    Mencius.proto:197-203
 *   Phase1a { round = 1; chosen_watermark = 2; }   Nack { round = 1; }                        :104-117, 266-271
 *
 * Decoders: as above (buf, buf_len, offsets, n); slot = the slot, or slot_start_inclusive of a range; slot_end =
 * slot_end_exclusive of a range (-1 otherwise); fields that do not apply are -1; any output array but kind, slot and
 * round may be NULL. */
int32_t fpx_wire_mencius_decode_proxy_leader_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets,
                                                     int32_t n, int32_t* kind, int32_t* slot, int32_t* slot_end,
                                                     int32_t* round, int32_t* is_noop, int64_t* value_off,
                                                     int32_t* value_len, int32_t* group_index, int32_t* acceptor_index,
                                                     int32_t* bad_index);
int32_t fpx_wire_mencius_decode_acceptor_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n,
                                                 int32_t* kind, int32_t* slot, int32_t* slot_end, int32_t* round,
                                                 int32_t* is_noop, int64_t* value_off, int32_t* value_len,
                                                 int32_t* chosen_watermark, int32_t* bad_index);
/* kind CHOSEN / CHOSEN_NOOP_RANGE / OTHER; round is not part of these messages (the array is not taken) */
int32_t fpx_wire_mencius_decode_replica_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n,
                                                int32_t* kind, int32_t* slot, int32_t* slot_end, int32_t* is_noop,
                                                int64_t* value_off, int32_t* value_len, int32_t* bad_index);
/* Encoders: one wrapped message each, return convention as above. */
int64_t fpx_wire_mencius_encode_proxy_leader_phase2a(uint8_t* out, int64_t cap, int32_t slot, int32_t round,
                                                     const uint8_t* value, int32_t value_len, int32_t is_noop);
int64_t fpx_wire_mencius_encode_acceptor_phase2a(uint8_t* out, int64_t cap, int32_t slot, int32_t round,
                                                 const uint8_t* value, int32_t value_len, int32_t is_noop);
int64_t fpx_wire_mencius_encode_proxy_leader_phase2a_noop_range(uint8_t* out, int64_t cap, int32_t slot_start,
                                                                int32_t slot_end, int32_t round);
int64_t fpx_wire_mencius_encode_acceptor_phase2a_noop_range(uint8_t* out, int64_t cap, int32_t slot_start,
                                                            int32_t slot_end, int32_t round);
int64_t fpx_wire_mencius_encode_acceptor_phase1a(uint8_t* out, int64_t cap, int32_t round, int32_t chosen_watermark);
int64_t fpx_wire_mencius_encode_proxy_leader_phase2b(uint8_t* out, int64_t cap, int32_t acceptor_index, int32_t slot,
                                                     int32_t round);
int64_t fpx_wire_mencius_encode_proxy_leader_phase2b_noop_range(uint8_t* out, int64_t cap, int32_t acceptor_group_index,
                                                                int32_t acceptor_index, int32_t slot_start,
                                                                int32_t slot_end, int32_t round);
int64_t fpx_wire_mencius_encode_replica_chosen(uint8_t* out, int64_t cap, int32_t slot, const uint8_t* value,
                                               int32_t value_len, int32_t is_noop);
int64_t fpx_wire_mencius_encode_replica_chosen_noop_range(uint8_t* out, int64_t cap, int32_t slot_start,
                                                          int32_t slot_end);
int64_t fpx_wire_mencius_encode_leader_nack(uint8_t* out, int64_t cap, int32_t round);

/* ---- EPaxos (shared/src/main/scala/frankenpaxos/epaxos/EPaxos.proto) -------------------------------------------
 *
 *   ReplicaInbound { oneof request { ClientRequest client_request = 1; PreAccept pre_accept = 2;
 *                    PreAcceptOk pre_accept_ok = 3; Accept accept = 4; AcceptOk accept_ok = 5; Commit commit = 6;
 *                    Prepare prepare = 7; PrepareOk prepare_ok = 8; Nack nack = 9; } }          EPaxos.proto:220-235
 *   Instance { replica_index = 1; instance_number = 2; }   Ballot { ordering = 1; replica_index = 2; }   :35-53
 *   CommandOrNoop { oneof value { Command command = 1; Noop noop = 2; } }                       EPaxos.proto:80-89
 *   InstancePrefixSetProto { numReplicas = 1; repeated IntPrefixSetProto int_prefix_set = 2; }  EPaxos.proto:97-104
 *   IntPrefixSetProto { watermark = 1; repeated int32 value = 2; }               compact/IntPrefixSet.proto:12-15
 *   PreAccept   { instance = 1; ballot = 2; command_or_noop = 3; sequence_number = 4; dependencies = 5; }   :113-123
 *   PreAcceptOk { instance = 1; ballot = 2; replica_index = 3; sequence_number = 4; dependencies = 5; }     :125-135
 *   Accept      { instance = 1; ballot = 2; command_or_noop = 3; sequence_number = 4; dependencies = 5; }   :137-147
 *   AcceptOk    { instance = 2; ballot = 3; replica_index = 7; }                                            :149-156
 *   Commit      { instance = 1; command_or_noop = 2; sequence_number = 3; dependencies = 4; }               :158-166
 *   Prepare     { instance = 1; ballot = 2; }                                                               :178-184
 *   PrepareOk   { ballot = 1; instance = 2; replica_index = 3; vote_ballot = 4; status = 5 (NotSeen 0 /
 *                 PreAccepted 1 / Accepted 2); optional command_or_noop = 6, sequence_number = 7,
 *                 dependencies = 8; }                                                                       :186-209
 *   Nack        { instance = 1; largest_ballot = 2; }                                                       :211-218
 *
 * One message as plain fields.  What a kind does not carry is -1 (is_noop: -1 = no CommandOrNoop present,
 * num_replicas: -1 = no dependencies present).  Dependencies: deps_watermark[l] for l < num_replicas and the
 * explicit ids (values_leader[j], values_id[j]), j < num_values.  ballot_* is the message's ballot (Nack:
 * largest_ballot). */
typedef struct {
  int32_t kind; /* FPX_WIRE_EPX_* */
  int32_t instance_leader, instance_number;
  int32_t ballot_ordering, ballot_replica;
  int32_t replica_index;                            /* PreAcceptOk, AcceptOk, PrepareOk */
  int32_t sequence_number;                          /* -1 with has_sequence_number = 0 */
  int32_t has_sequence_number;
  int32_t vote_ballot_ordering, vote_ballot_replica, status; /* PrepareOk */
  int32_t is_noop;                                  /* 1 Noop, 0 command, -1 none */
  const uint8_t* command;                           /* the serialised CommandOrNoop (as the decoder locates it) */
  int32_t command_len;
  int32_t num_replicas;                             /* -1: no dependencies */
  const int32_t* deps_watermark;
  int32_t num_values;
  const int32_t* values_leader;
  const int32_t* values_id;
} fpx_wire_epx_msg;

/* Encodes ONE ReplicaInbound (return convention as above; -(1 << 62) for a message that cannot be encoded: unknown
 * kind, a required part missing).  Explicit ids are written in the order given (ScalaPB writes `values.toSeq` of a
 * hash set: no canonical order exists; any order decodes to the same set). */
int64_t fpx_wire_epaxos_encode_replica_inbound(uint8_t* out, int64_t cap, const fpx_wire_epx_msg* msg);

/* Decodes n ReplicaInbound messages into SoA (every array has n entries unless said otherwise; any but kind may be
 * NULL).  deps_watermark is n x max_replicas (row i holds deps_num_replicas[i] <= max_replicas watermarks, the rest
 * 0; more replicas than max_replicas is FPX_EINVAL at that message).  Explicit ids of all messages back to back:
 * values of message i are values_leader / values_id [values_off[i] .. values_off[i + 1]) (values_off has n + 1
 * entries); if they do not fit values_cap the call returns FPX_ECAPACITY with values_off[n] = the capacity needed
 * (everything else is filled in) -- call again.  cmd_off / cmd_len locate the serialised CommandOrNoop in buf. */
int32_t fpx_wire_epaxos_decode_replica_inbound(const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n,
                                               int32_t max_replicas, int32_t* kind, int32_t* instance_leader,
                                               int32_t* instance_number, int32_t* ballot_ordering,
                                               int32_t* ballot_replica, int32_t* replica_index,
                                               int32_t* sequence_number, int32_t* vote_ballot_ordering,
                                               int32_t* vote_ballot_replica, int32_t* status, int32_t* is_noop,
                                               int64_t* cmd_off, int32_t* cmd_len, int32_t* deps_num_replicas,
                                               int32_t* deps_watermark, int64_t* values_off, int64_t values_cap,
                                               int32_t* values_leader, int32_t* values_id, int32_t* bad_index);

/* ---- EPaxos, the FOLDED form: what a message's dependencies are to the burst calls of include/fpx.h ---------------
 * The decoder above hands out every explicit id (a CSR over the tick, which takes a scan to build); the burst calls
 * (fpx_epx_leader_replies, fpx_epx_replica_inbox, ...) take a watermark row and ONE word, deps_values_end.  The folded
 * decoders give exactly that, from fixed-size state per message, and so run on the device too -- one parser source for
 * both sides (csrc/fpx_wire_epx_parse.hpp), which the decoder above runs as well.
 * The scalars are the decoder's above, field for field (kind, instance_*, ballot_*, replica_index, sequence_number,
 * vote_ballot_*, status, is_noop, cmd_off / cmd_len, deps_num_replicas), and deps_watermark is n x num_replicas, a
 * row padded with zeros; a message with more sets than num_replicas is malformed (whether deps_watermark is given or
 * not).  In place of the explicit ids:
 *   deps_values_end[i]  0 when message i has no dependencies or its own-leader column (instance_leader) has no
 *                       explicit ids, else the largest explicit id of that column + 1 (EPaxosNative.scala, ownEnd).
 *   deps_shape[i]       -1  no dependencies present.
 *                        1  the set is in the form every EPaxos burst call takes: no explicit id in any other column,
 *                           and the own column is either empty, or has watermark <= instance_number and the SET of
 *                           its ids is exactly instance_number + 1 .. deps_values_end - 1 (in any order, an id may
 *                           repeat: ScalaPB writes a hash set and every runtime reads duplicates into one).
 *                        0  anything else: an explicit id in a foreign column (top-k dependencies, k > 1), a gap, an
 *                           id at or below the instance number, an instance_leader outside the columns present, or
 *                           more than FPX_WIRE_EPX_FOLD_MAX explicit-id entries in the message (the cap makes the set
 *                           test an exact 64-bit mask and bounds one thread's work; explicit ids come from reordered
 *                           delivery on one channel and are few).  Such a message is the host decoder's.
 * The fold is made after the whole member is parsed: `dependencies` may precede `instance` in byte order.
 * kind is required, every other array may be NULL.  Errors as the decoder above (*bad_index is -1 when there is none). */
#define FPX_WIRE_EPX_FOLD_MAX 64
/* host, g++-compiled: runs on a machine without a GPU */
int32_t fpx_wire_epaxos_decode_replica_inbound_folded(
    const uint8_t* buf, int64_t buf_len, const int64_t* offsets, int32_t n, int32_t num_replicas, int32_t* kind,
    int32_t* instance_leader, int32_t* instance_number, int32_t* ballot_ordering, int32_t* ballot_replica,
    int32_t* replica_index, int32_t* sequence_number, int32_t* vote_ballot_ordering, int32_t* vote_ballot_replica,
    int32_t* status, int32_t* is_noop, int64_t* cmd_off, int32_t* cmd_len, int32_t* deps_num_replicas,
    int32_t* deps_watermark, int32_t* deps_values_end, int32_t* deps_shape, int32_t* bad_index);

/* The same ON THE DEVICE, the arrays as device pointers (the bytes and offsets may be page-locked host memory), enqueued
 * on the EPaxos context's stream; num_replicas = the context's n.  One thread per message.  d_kind is required, every
 * other output may be NULL -- but d_bad_index, which is ALWAYS written: -1 = none, otherwise the first bad offset, or,
 * all offsets being good, the first malformed message (a bad offset outranks a malformed message, as in the host
 * decoders).  A bad tick raises the context's status to FPX_EINVAL the way the EPaxos validation kernels do:
 * fpx_epx_sync reports it and the calls enqueued behind it apply nothing.  No host wait inside.  n < 2^30.  The outputs of
 * a failed decode are unspecified. */
struct fpx_epx;
int32_t fpx_wire_epaxos_decode_replica_inbound_dev(
    struct fpx_epx* epx, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_offsets, int32_t n, int32_t* d_kind,
    int32_t* d_instance_leader, int32_t* d_instance_number, int32_t* d_ballot_ordering, int32_t* d_ballot_replica,
    int32_t* d_replica_index, int32_t* d_sequence_number, int32_t* d_vote_ballot_ordering,
    int32_t* d_vote_ballot_replica, int32_t* d_status, int32_t* d_is_noop, int64_t* d_cmd_off, int32_t* d_cmd_len,
    int32_t* d_deps_num_replicas, int32_t* d_deps_watermark, int32_t* d_deps_values_end, int32_t* d_deps_shape,
    int32_t* d_bad_index);

/* One tick of hosted leaders (FPX_EPX_F_LEADER_STATE), bytes -> decisions: m serialised ReplicaInbound messages (in,
 * in_len, in_offsets[m + 1]; to[i] = the replica that received message i) -> copy up (host form) -> the decoder above
 * -> check -> fpx_epx_leader_replies_dev on the decoded arrays -> copy down.  The outputs are those of
 * fpx_epx_leader_replies[_dev] (include/fpx.h), unchanged, any of which may be NULL; the host form stages and holds them
 * exactly as fpx_epx_leader_replies does, the _dev form keeps the decoded arrays in scratch the context owns.
 * The tick holds PreAcceptOk, AcceptOk and Nack only (kinds 0, 1, 2 of fpx_epx_leader_replies); the caller routes by the
 * outer oneof tag, one byte.  A Nack carries no replica_index: the tick passes 0, which fpx_epx_leader_replies range-checks
 * and does not read for a Nack.  A defaultToSlowPath timer event (kind 3) has no bytes: the caller cuts its tick there and
 * passes the event through fpx_epx_leader_replies.
 * FPX_EINVAL with *bad_index (d_bad_index: always written; bad_index may be NULL) and NOTHING applied: a bad offset; a
 * malformed message; a message of any other kind, ClientRequest / OTHER included; a PreAcceptOk whose
 * deps_num_replicas is not the context's n or whose deps_shape is not 1 (the caller parses that one on the host).
 * Offsets are judged first, then the lowest offending index is reported.  A burst that decodes cleanly but that
 * fpx_epx_leader_replies itself refuses stays FPX_EINVAL with *bad_index = -1.  Otherwise every output and every piece
 * of device state is what fpx_epx_leader_replies leaves for the decoded burst, FPX_EFATAL_PROTOCOL (which skips a message
 * and applies the rest) included.  m = 0: FPX_OK, *num_decided = 0.  m < 2^30. */
int32_t fpx_wire_epx_leader_tick_dev(struct fpx_epx* epx, const uint8_t* d_in, int64_t in_len,
                                     const int64_t* d_in_offsets, int32_t m, const int32_t* d_to, int32_t* d_outcome,
                                     int32_t* d_out_seq, int32_t* d_out_deps, int32_t* d_out_values_end,
                                     int32_t* d_out_triple, int32_t* d_decided_index, int32_t* d_num_decided,
                                     int32_t* d_bad_index);
int32_t fpx_wire_epx_leader_tick(struct fpx_epx* epx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets,
                                 int32_t m, const int32_t* to, int32_t* outcome, int32_t* out_seq, int32_t* out_deps,
                                 int32_t* out_values_end, int32_t* out_triple, int32_t* decided_index,
                                 int32_t* num_decided, int32_t* bad_index);

/* ---- a replica's inbox from wire bytes ------------------------------------------------------------------------------
 * The counterpart of fpx_wire_epx_leader_tick for what peer replicas SEND hosted replicas: PreAccept, Accept, Commit and
 * Prepare.  Three of them carry a command, whose keys EPaxosNative.scala's classify reads with
 * KeyValueStoreInput.parseFrom and keyOf turns into ids on the JVM; here both happen on the device, against the context's
 * key table (include/fpx.h, fpx_epx_keys_enable -- without it every call below is FPX_EINVAL).
 *
 * The command's key list (csrc/fpx_epx_cmd_parse.hpp, one source for host and device), from the serialised CommandOrNoop
 * the decoders locate (cmd_off / cmd_len): CommandOrNoop { command = 1 | noop = 2 } -> Command.command (field 4) ->
 * KeyValueStoreInput { get_request = 1 { repeated key = 1 } | set_request = 2 { repeated { key = 1; value = 2 } } }.
 *   cmd_shape 1   canonical: exactly one member in CommandOrNoop; a Command with its four fields, `command` exactly once;
 *                 exactly one request member; every pair exactly one key (and a value); no unknown field and no other
 *                 wire type on the way down; no key longer than FPX_EPX_KEY_MAX_LEN.  is_noop / is_set say which, the keys
 *                 are reported in wire order.  A request without keys is shape 1 with an empty list, which the _mk calls
 *                 treat like a Noop.
 *   cmd_shape 0   anything else that is well-formed protobuf (ScalaPB would merge repeated members or take the last one;
 *                 Request.Empty; a required field missing): that frame is the JVM's, as deps_shape 0 frames are.  is_noop
 *                 = is_set = 0, no keys.
 *   malformed     truncated, a length running past its parent, a bad wire type: an error, as in the decoders.
 *   cmd_len[i] < 0: the message has no command (a Prepare): an empty list, is_noop = cmd_shape = -1.
 *
 * fpx_wire_epx_classify: the host classify (g++-compiled, no GPU): key_offsets[m + 1] and, for pair j of the burst, where
 * its key lies in buf (pair_off[j], pair_len[j]; either may be NULL) -- the caller maps strings to ids.  FPX_EINVAL with
 * *bad_index: the first malformed command (or one outside buf).  FPX_ECAPACITY: more than max_pairs pairs;
 * key_offsets[m] says how many.
 * fpx_wire_epx_key_hash: the table's hash (FNV-1a 64), for tests that choose colliding keys.
 *
 * fpx_wire_epx_classify_dev: the same on the device, and the ids: count -> scan -> parse again -> intern -> d_key_offsets
 * [m + 1] / d_keys[max_pairs], the CSR the _mk calls take; d_is_set as they take it.  d_result, 4 words: the bad index (-1
 * = none), num_pairs, the new keys and the new bytes this call interned.  No host wait; status through fpx_epx_sync:
 * FPX_EINVAL (a malformed command, d_result[0]) or FPX_ECAPACITY (more than max_pairs pairs -- d_result[1] says how many
 * -- or the key table's limits), NOTHING interned either way.  Shape-0 commands are reported, not refused.  buf_len <
 * 2^31, m <= FPX_EPX_INBOX_MAX, max_pairs <= FPX_EPX_MK_MAX_PAIRS.
 *
 * fpx_wire_epx_replica_tick[_dev]: one tick of hosted replicas, bytes -> outputs (Replica.scala:1159-1289, 1421-1511,
 * 1567-1575, 1632-1757 through fpx_epx_replica_inbox_mk).  m serialised ReplicaInbound messages, to[i] the replica that
 * received message i; the CommandTriple id of message i is triple_id[i], or with triple_id NULL triple_base + i (-1 for a
 * Prepare).  Stage 1, enqueued without a wait: the decoder, a check (PreAccept, Accept, Commit -- deps_num_replicas == n,
 * deps_shape == 1, cmd_shape == 1 -- and Prepare; the ballot's fields and the instance go in as decoded), the classify
 * above.  Then ONE host wait for the pair count and the status -- as fpx_epx_preaccept_mk_dev waits for its pair count,
 * so the tick CANNOT be captured into a HIP graph -- and stage 2: fpx_epx_replica_inbox_mk_dev's launches on the decoded
 * arrays.  An Accept or a Commit always passes its decoded dependencies (the by-id form is never produced).
 * The outputs are those of fpx_epx_replica_inbox_mk (any may be NULL; the host form holds them as that call does), then
 * the bad index and num_pairs.  Refusals, in this order, each with nothing applied to the command logs or the index:
 *   FPX_EINVAL, the lowest offending index, nothing interned: a bad offset (judged first); a malformed message or
 *                 command; a message of another kind; deps_shape or cmd_shape 0
 *   FPX_ECAPACITY, nothing interned: more than max_pairs pairs (num_pairs says how many), the key table's limits
 *   FPX_EINVAL, bad index -1: a burst that stage 1 accepts and fpx_epx_replica_inbox_mk_dev refuses (an instance outside
 *                 the log, a watermark rule, ...).  The keys of THAT burst stay interned: ids are never reused and the
 *                 table only grows.
 * m = 0 is FPX_OK.  The _dev form returns what enqueueing returns; its status comes through fpx_epx_sync. */
int32_t fpx_wire_epx_classify(const uint8_t* buf, int64_t buf_len, const int64_t* cmd_off, const int32_t* cmd_len, int32_t m,
                              int32_t max_pairs, int32_t* key_offsets, int64_t* pair_off, int32_t* pair_len,
                              uint8_t* is_set, int32_t* is_noop, int32_t* cmd_shape, int32_t* bad_index);
uint64_t fpx_wire_epx_key_hash(const uint8_t* bytes, int64_t len);
int32_t fpx_wire_epx_classify_dev(struct fpx_epx* epx, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_cmd_off,
                                  const int32_t* d_cmd_len, int32_t m, int32_t max_pairs, int32_t* d_key_offsets,
                                  int32_t* d_keys, uint8_t* d_is_set, int32_t* d_is_noop, int32_t* d_cmd_shape,
                                  int32_t* d_result);
int32_t fpx_wire_epx_replica_tick_dev(struct fpx_epx* epx, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets,
                                      int32_t m, const int32_t* d_to, int32_t triple_base, const int32_t* d_triple_id,
                                      int32_t max_pairs, int32_t* d_outcome, int32_t* d_out_ballot, int32_t* d_out_status,
                                      int32_t* d_out_deps, int32_t* d_out_values_end, int32_t* d_out_triple,
                                      int32_t* d_bad_index, int32_t* d_num_pairs);
int32_t fpx_wire_epx_replica_tick(struct fpx_epx* epx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets,
                                  int32_t m, const int32_t* to, int32_t triple_base, const int32_t* triple_id,
                                  int32_t max_pairs, int32_t* outcome, int32_t* out_ballot, int32_t* out_status,
                                  int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple, int32_t* bad_index,
                                  int32_t* num_pairs);

/* ---- a replica tick's replies as wire bytes ---------------------------------------------------------------------------
 * The outbound half of the tick above: what fpx_epx_replica_inbox[_mk] answers (outcome, out_ballot, out_status, out_deps
 * [m x n], out_values_end; include/fpx.h, FPX_EPX_RI_*) becomes the serialised ReplicaInbound messages the hosted replicas send
 * back, without the caller building one message at a time (EPaxosNative.scala, flushPeerInbox).  One emitter source for both
 * sides, csrc/fpx_wire_epx_emit.hpp: an encoded reply is, byte for byte, what fpx_wire_epaxos_encode_replica_inbound returns
 * for the same message.  Message i -- received by replica to[i], instance (leader[i], number[i]), the MESSAGE's ballot
 * (ballot_ordering[i], ballot_replica[i]) -- by outcome[i]:
 *   IGNORED, LEARNT                    no reply                                                          reply_kind 0
 *   PRE_ACCEPT_OK, PRE_ACCEPT_OK_AGAIN PreAcceptOk(instance, the message's ballot, to[i], 0, deps): deps = the n watermarks of
 *                                      row i, and in the own-leader column (l == leader[i]) the explicit ids number + 1 ..
 *                                      out_values_end - 1, ascending, when out_values_end > 0.      reply_kind 1 -- but 2
 *                                      (deferred) when out_deps[i * n] < 0 (a triple stored by id: the caller has its
 *                                      dependencies) or the own column would carry more than FPX_WIRE_EPX_FOLD_MAX ids
 *   ACCEPT_OK, ACCEPT_OK_AGAIN         AcceptOk(instance, the message's ballot, to[i])                   reply_kind 1
 *   NACK                               Nack(instance, Ballot(out_ballot >> 3, out_ballot & 7))           reply_kind 1
 *   PREPARE_OK                         out_status 0: PrepareOk(the message's ballot, instance, to[i], voteBallot, NotSeen)
 *                                      without the three optional fields; voteBallot = (-1, -1), the reference's nullBallot,
 *                                      when out_ballot < 0.  reply_kind 1.  Any other out_status: reply_kind 2, the reply
 *                                      carries the stored triple's CommandOrNoop, whose bytes live with the caller (but see
 *                                      "with the command store" below)
 *   COMMIT_BACK                        reply_kind 2, for the same reason
 * A deferred record is no error: it contributes no bytes and the caller builds that one reply from the struct-of-arrays
 * outputs, as it does today.  (The steady traffic of a replica is outcomes 1, 3 and 7; the deferred ones are recovery and
 * commit-back.)  The records are not validated beyond outcome being in 0 .. 8.
 *   bytes    the reply of message i is out[out_offsets[i] .. out_offsets[i + 1]), empty for kinds 0 and 2: offsets are per
 *            MESSAGE, m + 1 of them, nothing is compacted (reply i goes to the sender of message i).
 *   totals   4 words, ALWAYS written: the replies encoded, the bytes needed, the records deferred, and the first record with
 *            an unknown outcome (-1 = none; this context has no error-detail call, so the index travels here).
 *   FPX_ECAPACITY  the bytes needed exceed cap (or, on the device, reach 4 GiB in one call: its scan is 32 bits wide -- cut the
 *            burst): no byte of out and no out_offsets entry beyond [0] (= 0) is written, reply_kind
 *            is not written; totals say what to allocate.  cap == 0 with out == NULL is the sizing call.
 *   FPX_EINVAL     an outcome outside 0 .. 8: totals[3] names the first, nothing else is written but out_offsets[0] = 0.
 *   m == 0   FPX_OK, totals 0, out_offsets[0] = 0.
 * A NULL required array, n < 1, negative sizes or m > FPX_EPX_INBOX_MAX: FPX_EINVAL at once.
 * FPX_WIRE_EPX_REPLY_MAX: no encoded reply is longer, given what fpx_epx_replica_inbox puts out -- n <= 7, at most 64 explicit
 * ids, a ballot ordering below 2^27, every other number a non-negative int32.  It is a PreAcceptOk: 3 bytes of wrapper, the
 * instance 10, the ballot 9, replica_index and sequence_number 2 each, and 3 + 443 of dependencies (numReplicas 2, six columns
 * of 8, the own column 3 + 6 + 64 x 6).  cap >= m x FPX_WIRE_EPX_REPLY_MAX makes FPX_ECAPACITY unreachable.
 *
 * fpx_wire_epx_encode_replica_replies: the host batch encoder, g++-compiled, no GPU.
 * fpx_wire_epx_encode_replica_replies_dev: the same arrays as device pointers (n is the context's), enqueued on the context's
 * stream, no host wait inside -- so, once the context's scratch is sized (the first call with a larger m than any before
 * allocates 4 bytes per record: run one call with the largest m outside the capture), it can be captured into a HIP
 * graph.  Both errors above are PER-CALL codes: they come through fpx_epx_sync, which returns and clears them like any status
 * (a status raised by another call outranks them), but no later call on the context stands back behind them.  A context that
 * is in its "apply nothing" state when the encoder runs (a refused burst in front of it): totals 0, out_offsets[0] = 0,
 * nothing else.
 *
 * fpx_wire_epx_replica_tick_bytes[_dev]: fpx_wire_epx_replica_tick's stages, unchanged, then the encoder on the decoded
 * arrays the tick holds in scratch and on the inbox outputs: frames in, the frames to send back out.  The six struct-of-
 * arrays outputs are ALL optional here -- a caller needs them for its deferred records (reply_kind 2); what it leaves NULL
 * the tick keeps in scratch of its own and never copies down.  Refusals are exactly fpx_wire_epx_replica_tick's, in its order,
 * each with nothing applied and nothing encoded (totals 0, out_offsets[0] = 0; the host form leaves every other output array
 * as it was).  FPX_ECAPACITY from the ENCODER means the tick WAS applied: the struct-of-arrays outputs, where requested, are
 * valid and the caller encodes from them (fpx_wire_epx_encode_replica_replies); totals[1] > out_cap tells this
 * FPX_ECAPACITY from stage 1's, whose totals are 0.  Like its sibling the tick waits once on the host for the pair count and
 * cannot be captured into a graph.  m = 0 is FPX_OK.
 * The host form goes through the staging driver like its sibling.  Its copy down moves 32 bytes of totals, 8 bytes of bad
 * index and pair count, then -- on FPX_OK -- 8 (m + 1) bytes of offsets, m bytes of kinds and the totals[1] bytes of the
 * replies, NOT out_cap bytes; plus 4 bytes per message for each requested struct-of-arrays output (4 n for out_deps), against
 * the (5 + n) x 4 bytes per message fpx_wire_epx_replica_tick moves for all six.  out_cap bytes are staged on the device.
 * Deviations from the issue's proposal: totals has a fourth word; reply_kind is bytes.
 *
 * ---- with the command store (include/fpx.h, fpx_epx_cmds_*) ----
 * Everything above holds for a context without the store and for the two encoders above on any context.  The _cmds forms take
 * out_triple as well and a command source -- triple t's serialised CommandOrNoop is arena[cmd_off[t] .. cmd_off[t] + cmd_len[t]),
 * cmd_off[t] < 0 = no bytes, t in [0, max_triples) -- and encode the two replies that carry a stored command:
 *   COMMIT_BACK                        Commit(instance, the stored CommandOrNoop verbatim, 0, deps)       reply_kind 1
 *   PREPARE_OK, out_status 2 / 3       PrepareOk(the message's ballot, instance, to[i], voteBallot, PreAccepted / Accepted
 *                                      (wire status out_status - 1), the stored CommandOrNoop, 0, deps)  reply_kind 1
 * when out_triple[i] is in range and has bytes, out_deps[i * n] >= 0 and the own column has at most FPX_WIRE_EPX_FOLD_MAX
 * explicit ids (deps as a PreAcceptOk's, above); otherwise the record stays deferred (reply_kind 2), as does a PREPARE_OK
 * of any other out_status but 0.  What is left deferred with the store: dependencies known by id only, more than 64 explicit
 * ids, a triple the store skipped or never saw.
 * FPX_WIRE_EPX_CMD_REPLY_MAX(cmd_len): no reply that carries a command of cmd_len <= FPX_EPX_CMD_MAX_LEN bytes is longer, under
 * the assumptions of FPX_WIRE_EPX_REPLY_MAX.  It is a PrepareOk whose voteBallot is nullBallot: the ballot 9, the instance 10,
 * replica_index 2, voteBallot 24 (two ten-byte varints), status 2, the command 1 + varint(cmd_len) + cmd_len,
 * sequence_number 2 and 3 + 443 of dependencies: 496 + varint(cmd_len) + cmd_len of inner bytes, under 1 + varint(inner) of
 * wrapper.
 * fpx_wire_epx_encode_replica_replies_cmds: the host batch encoder with the store as plain arrays; cmd_off == cmd_len == NULL
 * and max_triples == 0 is no store, exactly fpx_wire_epx_encode_replica_replies.
 * fpx_wire_epx_encode_replica_replies_cmds_dev: the _dev arguments and d_out_triple (required for m > 0); the source is the
 * context's store (a context without one: exactly the _dev call).  No host wait, the same capture rules; the store's arrays
 * are read, so a put enqueued in front of it on the stream is seen.
 * On a context with the store fpx_wire_epx_replica_tick[_dev] and fpx_wire_epx_replica_tick_bytes[_dev] PUT the burst's commands
 * (the decoded cmd_off / cmd_len, triple_id or triple_base + i) behind stage 2, standing back behind its status: a burst
 * that is refused anywhere stores nothing.  The put takes the command of EVERY decoded frame of an applied burst, whatever its
 * outcome: a frame the inbox answers with a Nack or ignores leaves its bytes in the arena too, under its triple id, although
 * that triple never enters the command log (the arena is sized by the frames received, not by the instances stored).  The
 * bytes tick then encodes with the store, so a Commit and a Prepare of one
 * instance in ONE burst give a reply that carries that burst's bytes.  totals, reply_kind and the refusals keep their meaning;
 * a reply may now be as long as FPX_WIRE_EPX_CMD_REPLY_MAX(cmd_len), so m x FPX_WIRE_EPX_REPLY_MAX no longer rules FPX_ECAPACITY
 * out: that code from the encoder still means the tick was applied, totals[1] says what to allocate, and the caller re-encodes
 * with fpx_wire_epx_encode_replica_replies_cmds_dev from the struct-of-arrays outputs it asked for. */
#define FPX_WIRE_EPX_REPLY_MAX 472
#define FPX_WIRE_VARINT_LEN21(v) ((v) < (1 << 7) ? 1 : (v) < (1 << 14) ? 2 : 3) /* v < 2^21 */
#define FPX_WIRE_EPX_CMD_REPLY_INNER(cmd_len) (496 + FPX_WIRE_VARINT_LEN21(cmd_len) + (cmd_len))
#define FPX_WIRE_EPX_CMD_REPLY_MAX(cmd_len) \
  (1 + FPX_WIRE_VARINT_LEN21(FPX_WIRE_EPX_CMD_REPLY_INNER(cmd_len)) + FPX_WIRE_EPX_CMD_REPLY_INNER(cmd_len))
int32_t fpx_wire_epx_encode_replica_replies_cmds(int32_t n, int32_t m, const int32_t* to, const int32_t* leader,
                                                 const int32_t* number, const int32_t* ballot_ordering,
                                                 const int32_t* ballot_replica, const int32_t* outcome, const int32_t* out_ballot,
                                                 const int32_t* out_status, const int32_t* out_deps, const int32_t* out_values_end,
                                                 const int32_t* out_triple, const int64_t* cmd_off, const int32_t* cmd_len,
                                                 const uint8_t* arena, int32_t max_triples, uint8_t* out, int64_t cap,
                                                 int64_t* out_offsets, uint8_t* reply_kind, int64_t* totals);
int32_t fpx_wire_epx_encode_replica_replies_cmds_dev(struct fpx_epx* epx, int32_t m, const int32_t* d_to, const int32_t* d_leader,
                                                     const int32_t* d_number, const int32_t* d_ballot_ordering,
                                                     const int32_t* d_ballot_replica, const int32_t* d_outcome,
                                                     const int32_t* d_out_ballot, const int32_t* d_out_status,
                                                     const int32_t* d_out_deps, const int32_t* d_out_values_end,
                                                     const int32_t* d_out_triple, uint8_t* d_out, int64_t cap,
                                                     int64_t* d_out_offsets, uint8_t* d_reply_kind, int64_t* d_totals);
int32_t fpx_wire_epx_encode_replica_replies(int32_t n, int32_t m, const int32_t* to, const int32_t* leader, const int32_t* number,
                                            const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* outcome,
                                            const int32_t* out_ballot, const int32_t* out_status, const int32_t* out_deps,
                                            const int32_t* out_values_end, uint8_t* out, int64_t cap, int64_t* out_offsets,
                                            uint8_t* reply_kind, int64_t* totals);
int32_t fpx_wire_epx_encode_replica_replies_dev(struct fpx_epx* epx, int32_t m, const int32_t* d_to, const int32_t* d_leader,
                                                const int32_t* d_number, const int32_t* d_ballot_ordering,
                                                const int32_t* d_ballot_replica, const int32_t* d_outcome,
                                                const int32_t* d_out_ballot, const int32_t* d_out_status,
                                                const int32_t* d_out_deps, const int32_t* d_out_values_end, uint8_t* d_out,
                                                int64_t cap, int64_t* d_out_offsets, uint8_t* d_reply_kind, int64_t* d_totals);
int32_t fpx_wire_epx_replica_tick_bytes_dev(struct fpx_epx* epx, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets,
                                            int32_t m, const int32_t* d_to, int32_t triple_base, const int32_t* d_triple_id,
                                            int32_t max_pairs, uint8_t* d_out, int64_t out_cap, int64_t* d_out_offsets,
                                            uint8_t* d_reply_kind, int64_t* d_totals, int32_t* d_outcome, int32_t* d_out_ballot,
                                            int32_t* d_out_status, int32_t* d_out_deps, int32_t* d_out_values_end,
                                            int32_t* d_out_triple, int32_t* d_bad_index, int32_t* d_num_pairs);
int32_t fpx_wire_epx_replica_tick_bytes(struct fpx_epx* epx, const uint8_t* in, int64_t in_len, const int64_t* in_offsets,
                                        int32_t m, const int32_t* to, int32_t triple_base, const int32_t* triple_id,
                                        int32_t max_pairs, uint8_t* out, int64_t out_cap, int64_t* out_offsets,
                                        uint8_t* reply_kind, int64_t* totals, int32_t* outcome, int32_t* out_ballot,
                                        int32_t* out_status, int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple,
                                        int32_t* bad_index, int32_t* num_pairs);

#ifdef __cplusplus
}
#endif
#endif /* FPX_WIRE_H */
