// Native.scala -- the reference-side binding a frankenpaxos maintainer would add (source only: no
// JDK / scalac in this image).  Drop into jvm/src/main/scala/frankenpaxos/gpu/ of the reference.
//
// `Native` is the JNI surface of frankenpaxos_amd/jni/fpx_jni.c.  `GpuPhase2Engine` owns one libfpx context --
// the acceptors of every group plus the proxy leader's tallies -- and maps the unbounded log onto the
// context's window of rows.  Two thin actors put it behind the unchanged Actor/Transport trait surface:
//   * `GpuProxyLeader` stands at a proxy leader's address (with `remoteAcceptors = true` among the reference's own
//     Acceptor actors: Phase2as are opened and forwarded, the acceptors' Phase2bs tallied on the device once per
//     tick); with every acceptor in the engine its `receive` only ENQUEUES Phase2a messages, a
//     zero-delay Transport timer (the "tick") flushes the queue through ONE native call and then `send`s the
//     Nack / Chosen messages the Scala handlers would have sent (multipaxos/Acceptor.scala:192-219,
//     multipaxos/ProxyLeader.scala:246-253);
//   * `GpuAcceptor` stands at EVERY acceptor address (all instances share the engine): the Leader's Phase1a
//     (multipaxos/Leader.scala:231, 410-420) is answered with the Phase1b / Nack of
//     multipaxos/Acceptor.scala:148-182, built from fpx_acceptor_phase1a + fpx_acceptor_phase1b_info, which
//     is what the unchanged Leader.handlePhase1b (Leader.scala:504-577) needs to recover and re-propose; and the
//     read path -- MaxSlotRequest / BatchMaxSlotRequest are answered with Acceptor.maxVotedSlot (Acceptor.scala:
//     222-254), which the engine follows per acceptor (GpuPhase2Engine.maxVotedSlot).
//     Among the reference's own ProxyLeader actors -- GPU acceptors, everything else the reference's -- every Phase2a
//     arrives once per acceptor address (ProxyLeader.scala:190-215): `receive` only ENQUEUES, and one tick hands the
//     whole burst, Phase2as, Phase1as and reads interleaved, to ONE native call (fpx_acceptor_inbox;
//     GpuPhase2Engine.flushInbox).
package frankenpaxos.gpu

import frankenpaxos.Actor
import frankenpaxos.Chan
import frankenpaxos.Logger
import frankenpaxos.multipaxos._
import frankenpaxos.roundsystem.RoundSystem
import scala.collection.mutable

object Native {
  System.loadLibrary("fpxjni") // libfpxjni.so -> libfpx.so

  // status codes of include/fpx.h
  val OK = 0; val EINVAL = 1; val EFATAL_UNKNOWN_SLOTROUND = 2
  // message kinds of include/fpx_wire.h (the `kind` arrays of proxyPhase2bMsgs / menciusProxyPhase2bMsgs)
  val WIRE_PHASE2B = 2; val WIRE_PHASE2B_NOOP_RANGE = 7
  // ... and of acceptorInbox's kind / replyKind
  val WIRE_OTHER = 0; val WIRE_PHASE2A = 1; val WIRE_PHASE1A = 3; val WIRE_NACK = 5; val WIRE_PHASE1B = 9
  val WIRE_PHASE2A_NOOP_RANGE = 6       // menciusAcceptorInbox
  val WIRE_MAX_SLOT_REQUEST = 10; val WIRE_BATCH_MAX_SLOT_REQUEST = 11

  @native def create(cfg: Array[Int]): Long // < 0: -status
  @native def destroy(handle: Long): Int
  @native def acceptorPhase2a(handle: Long, n: Int, slot: Array[Int], round: Array[Int],
                              value: Array[Int], targetMask: Array[Long], voteBits: Array[Long],
                              nackBits: Array[Long], nackRound: Array[Int]): Int
  @native def proxyOpen(handle: Long, n: Int, slot: Array[Int], round: Array[Int],
                        value: Array[Int], isNew: Array[Byte]): Int
  @native def proxyPhase2b(handle: Long, n: Int, slot: Array[Int], round: Array[Int],
                           voteBits: Array[Long], newlyChosen: Array[Byte],
                           chosenRound: Array[Int], chosenValue: Array[Int]): Int
  // the same for ONE Phase2b per (acceptor, slot) as remote acceptors send them, any order, duplicates allowed
  // (fpx_proxy_phase2b_msgs): the fold into rows runs on the device; a row's outcome is at its first message.  kind
  // (FPX_WIRE_*; null = all Phase2b) and groupIndex (null = 0) may be null; gridCols = 0 unless the quorums are a grid
  @native def proxyPhase2bMsgs(handle: Long, n: Int, kind: Array[Int], groupIndex: Array[Int],
                               acceptorIndex: Array[Int], slot: Array[Int], round: Array[Int], gridCols: Int,
                               newlyChosen: Array[Byte], chosenRound: Array[Int], chosenValue: Array[Int]): Int
  // multipaxos.Acceptor's inbox for a burst of per-acceptor messages in delivery order, the kinds interleaved
  // (fpx_acceptor_inbox; Acceptor.scala:148-254): kind = WIRE_PHASE2A / WIRE_PHASE1A / WIRE_MAX_SLOT_REQUEST /
  // WIRE_BATCH_MAX_SLOT_REQUEST / WIRE_OTHER (skipped); (groupIndex, acceptorIndex) = who received message i, local to the
  // context (groupIndex null = 0; gridCols as in proxyPhase2bMsgs).  replyKind: 0 / WIRE_PHASE2B / WIRE_NACK /
  // WIRE_PHASE1B / WIRE_MAX_SLOT_REQUEST; replyValue: the Nack's round, the vote's or promise's round, the read's
  // maxVotedSlot (a ROW of the window here: GpuPhase2Engine keeps slots itself).  Phase1b.info is not produced
  @native def acceptorInbox(handle: Long, n: Int, kind: Array[Int], groupIndex: Array[Int], acceptorIndex: Array[Int],
                            slot: Array[Int], round: Array[Int], value: Array[Int], gridCols: Int,
                            replyKind: Array[Int], replyValue: Array[Int]): Int
  // mencius.Acceptor.receive for a burst of per-acceptor messages in delivery order, Phase2aNoopRanges among them
  // (fpx_mencius_acceptor_inbox; mencius/Acceptor.scala:142-291): slot = a Phase2a's slot or a range's start, slotEnd = a
  // range's end; groupIndex = leader group * numGroups + acceptor group; groupIndex, replyKind, replyValue may be null
  @native def menciusAcceptorInbox(handle: Long, n: Int, kind: Array[Int], groupIndex: Array[Int],
                                   acceptorIndex: Array[Int], slot: Array[Int], slotEnd: Array[Int], round: Array[Int],
                                   value: Array[Int], replyKind: Array[Int], replyValue: Array[Int]): Int
  // mencius.ProxyLeader.handlePhase2aNoopRange bookkeeping for n ranges in one call (fpx_proxy_open_noop_ranges)
  @native def proxyOpenNoopRanges(handle: Long, n: Int, slotStart: Array[Int], slotEnd: Array[Int],
                                  round: Array[Int], isNew: Array[Byte]): Int
  // Mencius: ONE Phase2b / Phase2bNoopRange per (acceptor, key) as remote Mencius acceptors send them, both kinds
  // interleaved in delivery order (fpx_mencius_proxy_phase2b_msgs; mencius/ProxyLeader.scala:305-411).  kind (FPX_WIRE_*;
  // null = all Phase2b), groupIndex (null = 0; a range message's acceptor group) and slotEnd (null = no range message)
  // may be null; a row's outcome is at its first message, chosenValue = -1 for a ChosenNoopRange
  @native def menciusProxyPhase2bMsgs(handle: Long, n: Int, kind: Array[Int], groupIndex: Array[Int],
                                      acceptorIndex: Array[Int], slot: Array[Int], slotEnd: Array[Int],
                                      round: Array[Int], newlyChosen: Array[Byte], chosenRound: Array[Int],
                                      chosenValue: Array[Int]): Int
  // the same as one tick: the newly chosen records (kind, slot, slotEnd or -1, round, value id or -1) compacted on the
  // device in message order into arrays of outCap records; outCount(0) = how many there are (ECAPACITY = 5: the tick was
  // applied, the first outCap records are written)
  @native def menciusPhase2bTick(handle: Long, n: Int, kind: Array[Int], groupIndex: Array[Int],
                                 acceptorIndex: Array[Int], slot: Array[Int], slotEnd: Array[Int], round: Array[Int],
                                 outKind: Array[Int], outSlot: Array[Int], outSlotEnd: Array[Int],
                                 outRound: Array[Int], outValue: Array[Int], outCap: Int, outCount: Array[Int]): Int
  @native def phase2Fused(handle: Long, n: Int, slot: Array[Int], round: Array[Int],
                          value: Array[Int], targetMask: Array[Long], chosen: Array[Byte],
                          chosenRound: Array[Int], chosenValue: Array[Int], nackRound: Array[Int]): Int
  @native def quorumEval(cfg: Array[Int], n: Int, nodes: Array[Long], strict: Int,
                         out: Array[Byte]): Int

  // page-locked batches: direct buffers over fpx_host_alloc memory (fill through asIntBuffer /
  // asLongBuffer views in ByteOrder.nativeOrder), DMA'd without pinning or copying
  @native def hostAlloc(bytes: Long): java.nio.ByteBuffer // null on failure
  @native def hostFree(buffer: java.nio.ByteBuffer): Int
  @native def phase2FusedDirect(handle: Long, n: Int, slot: java.nio.ByteBuffer,
                                round: java.nio.ByteBuffer, value: java.nio.ByteBuffer,
                                targetMask: java.nio.ByteBuffer, chosen: java.nio.ByteBuffer,
                                chosenRound: java.nio.ByteBuffer, chosenValue: java.nio.ByteBuffer,
                                nackRound: java.nio.ByteBuffer): Int

  // up to 3 ticks in flight on page-locked batches: submit returns a ticket (< 0: -status), wait its status; the
  // PCIe transfers of one tick hide behind the fused step of its neighbours (fpx_phase2_fused_submit / _wait)
  @native def phase2FusedSubmitDirect(handle: Long, n: Int, slot: java.nio.ByteBuffer,
                                      round: java.nio.ByteBuffer, value: java.nio.ByteBuffer,
                                      targetMask: java.nio.ByteBuffer, chosen: java.nio.ByteBuffer,
                                      chosenRound: java.nio.ByteBuffer, chosenValue: java.nio.ByteBuffer,
                                      nackRound: java.nio.ByteBuffer): Int
  @native def phase2FusedWait(handle: Long, ticket: Int): Int

  // one proxy-leader tick bytes to bytes (fpx_wire_phase2_tick): n serialised ProxyLeaderInbound{Phase2a} in `in`
  // (inLen bytes, inOffsets: n + 1 longs) -> the tick's ReplicaInbound{Chosen} messages in `out` (out.capacity >= inLen
  // always suffices; outOffsets: n + 1 longs) and the Nack rounds (n ints, may be null); every buffer a direct buffer
  // over hostAlloc memory in native byte order.  counts(0) = messages written, (1) = bytes needed, (2) = bad index
  @native def wirePhase2Tick(handle: Long, in: java.nio.ByteBuffer, inLen: Long, inOffsets: java.nio.ByteBuffer,
                             n: Int, out: java.nio.ByteBuffer, outOffsets: java.nio.ByteBuffer,
                             nackRound: java.nio.ByteBuffer, counts: Array[Long]): Int

  // the rows around the fused step
  @native def roundLeader(numLeaders: Int, round: Int): Int // < 0: -status (numLeaders < 1)
  @native def acceptorPhase1a(handle: Long, group: Int, round: Int, chosenWatermark: Int,
                              targetMask: Array[Long], bits: Array[Long]): Int
  @native def leaderPhase1bScan(handle: Long, chosenWatermark: Int, numGroups: Int,
                                quorumMasks: Array[Long], cap: Int, maxSlot: Array[Int],
                                safeRound: Array[Int], safeValue: Array[Int]): Int
  @native def replicaChosen(handle: Long, n: Int, slot: Array[Int], value: Array[Int],
                            mask: Array[Byte], state: Array[Int]): Int
  @native def replicaChosenNoopRange(handle: Long, slotStart: Int, slotEnd: Int,
                                     state: Array[Int]): Int
  // a burst of Chosen / ChosenNoopRange messages in delivery order (kind as fpx_wire.h numbers it)
  @native def replicaChosenMsgs(handle: Long, n: Int, kind: Array[Int], slot: Array[Int],
                                slotEnd: Array[Int], value: Array[Int], mask: Array[Byte],
                                state: Array[Int]): Int
  // a MultiPaxos replica's burst of Chosens and reads in delivery order (fpx_replica_inbox): execCount / replySlot per
  // message, order = the reads that ran in run order then the still-deferred ones, counts = {reads, ran, W0, W1}
  @native def replicaInbox(handle: Long, n: Int, kind: Array[Int], slot: Array[Int], value: Array[Int],
                           mask: Array[Byte], execCount: Array[Int], replySlot: Array[Int], order: Array[Int],
                           counts: Array[Int], state: Array[Int]): Int
  // Mencius noop ranges: n per call (the fused step), and the unfused pieces for one range
  @native def noopRangesFused(handle: Long, n: Int, numGroups: Int, slotStart: Array[Int],
                              slotEnd: Array[Int], round: Array[Int], targetMasks: Array[Long],
                              voteBits: Array[Long], nackBits: Array[Long], nackRound: Array[Int],
                              isNew: Array[Byte], chosen: Array[Byte]): Int
  @native def acceptorPhase2aNoopRange(handle: Long, slotStart: Int, slotEnd: Int, round: Int,
                                       numGroups: Int, targetMasks: Array[Long],
                                       bits: Array[Long], nackRound: Array[Int]): Int
  @native def proxyOpenNoopRange(handle: Long, slotStart: Int, slotEnd: Int, round: Int,
                                 isNew: Array[Byte]): Int
  @native def proxyPhase2bNoopRange(handle: Long, slotStart: Int, slotEnd: Int, round: Int,
                                    numGroups: Int, voteBits: Array[Long],
                                    newlyChosen: Array[Byte]): Int
  @native def epxCreate(numReplicas: Int, numKeys: Int, device: Int): Long // < 0: -status
  @native def epxDestroy(handle: Long): Int
  @native def epxPreaccept(handle: Long, m: Int, numReplicas: Int, leader: Array[Int],
                           number: Array[Int], key: Array[Int], isSet: Array[Byte],
                           respMask: Array[Byte], seenMask: Array[Byte], rank: Array[Int],
                           fast: Array[Byte], deps: Array[Int], leaderDeps: Array[Int],
                           ownValuesEnd: Array[Int]): Int
  // EPaxos on the command log (Replica.cmdLog): Prepare, Accept, handlePreAccept with ballots / Nacks / re-sent
  // replies.  replies packs the per-message reply bit sets back to back (m bytes each), see fpx_jni.c
  @native def epxCreateWithLog(numReplicas: Int, numKeys: Int, device: Int, numInstances: Int): Long
  @native def epxPrepare(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int],
                         ballotOrdering: Array[Int], ballotReplica: Array[Int], targetMask: Array[Byte],
                         replies: Array[Byte], nackBallot: Array[Int], prepareOk: Array[Int]): Int
  // Replica.handlePrepareOk: decision = action | source | triple (3 x m); action 0 wait, 1 Accept phase with the
  // triple, 2 pre-accept its command again, 3 pre-accept a Noop; asIntended = 0 evaluates :1810 / :1831 as written
  @native def epxHandlePrepareOks(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int],
                                  ballotOrdering: Array[Int], ballotReplica: Array[Int], respMask: Array[Byte],
                                  prepareOk: Array[Int], asIntended: Int, decision: Array[Int]): Int
  @native def epxAccept(handle: Long, m: Int, leader: Array[Int], number: Array[Int],
                        ballotOrdering: Array[Int], ballotReplica: Array[Int], tripleId: Array[Int],
                        key: Array[Int], isSet: Array[Byte],
                        targetMask: Array[Byte], replies: Array[Byte], nackBallot: Array[Int]): Int
  // Replica.handleCommit at the replicas of targetMask: deps m x n + depsValuesEnd m, or both null (triple by id alone)
  @native def epxHandleCommit(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int],
                              tripleId: Array[Int], key: Array[Int], isSet: Array[Byte], deps: Array[Int],
                              depsValuesEnd: Array[Int], targetMask: Array[Byte]): Int
  // Replica.execute on the device: the dependency graph of the committed instances handed in (dense columns first(l) ..
  // first(l) + count(l) - 1), strongly connected components in reverse topological order.  order / component: m each;
  // counts = (executed, components, needsHostPath)
  @native def epxExecute(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], deps: Array[Int],
                         depsValuesEnd: Array[Int], committed: Array[Byte], first: Array[Int], count: Array[Int],
                         order: Array[Int], component: Array[Int], counts: Array[Int]): Int
  @native def epxHandlePreaccept(handle: Long, m: Int, numReplicas: Int, leader: Array[Int],
                                 number: Array[Int], ballotOrdering: Array[Int],
                                 ballotReplica: Array[Int], key: Array[Int], isSet: Array[Byte],
                                 tripleId: Array[Int], depsIn: Array[Int], depsInValuesEnd: Array[Int],
                                 targetMask: Array[Byte], replies: Array[Byte], nackBallot: Array[Int],
                                 replyDeps: Array[Int], replyEndTriple: Array[Int]): Int
  // ---- the leader half of an instance (include/fpx.h, FPX_EPX_F_LEADER_STATE): a context that also keeps
  // Replica.leaderStates, for replicas that lead among peers in other processes
  @native def epxCreateWithLeaderState(numReplicas: Int, numKeys: Int, device: Int, numInstances: Int): Long
  // transitionToPreAcceptPhase at replica at(i) in ballot (ballotOrdering(i), at(i)) (epaxos/Replica.scala:633-729), key -1 =
  // Noop; deps (m x n) / depsValuesEnd (m): the dependencies of the PreAccept to send.  9 (FPX_EFATAL_PROTOCOL): a message
  // the reference would have died on was skipped
  @native def epxLead(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], at: Array[Int],
                      ballotOrdering: Array[Int], key: Array[Int], isSet: Array[Byte], tripleId: Array[Int],
                      avoidFastPath: Array[Byte], deps: Array[Int], depsValuesEnd: Array[Int]): Int
  // one burst of PreAcceptOk (kind 0) / AcceptOk (1) / Nack (2) messages and fired defaultToSlowPath timers (3) at hosted
  // leaders, in delivery order (handlePreAcceptOk :1291-1419, handleAcceptOk :1514-1565, handleNack :1577-1630).  outcome (m):
  // 0 ignored, 1 waiting, 2 start the defaultToSlowPath timer, 3 fast commit, 4 Accept phase, 5 slow commit, 6 Nack: start
  // the recover-instance timer, 7 Nack ignored, 8 skipped (fatal in the reference); triple = sequence number | values end |
  // triple id (3 x m) and outDeps (m x n): the triple of the Commit / Accept to send for 3 / 4 / 5; decided (m + 1): how
  // many messages have such an outcome, then their indices
  @native def epxLeaderReplies(handle: Long, m: Int, numReplicas: Int, kind: Array[Int], to: Array[Int], leader: Array[Int],
                               number: Array[Int], ballotOrdering: Array[Int], ballotReplica: Array[Int],
                               replicaIndex: Array[Int], sequenceNumber: Array[Int], deps: Array[Int],
                               depsValuesEnd: Array[Int], outcome: Array[Int], triple: Array[Int], outDeps: Array[Int],
                               decided: Array[Int]): Int
  // the same burst as serialised ReplicaInbound messages, bytes -> decisions without the host parsing a byte
  // (include/fpx_wire.h, fpx_wire_epx_leader_tick): in (inLen bytes), inOffsets (m + 1 longs) and to (m ints: the replica that
  // received message i) are direct buffers in native byte order, as wirePhase2Tick's; the outputs are epxLeaderReplies'.
  // PreAcceptOk, AcceptOk and Nack only -- a fired defaultToSlowPath timer has no bytes: cut the tick there and pass the
  // event through epxLeaderReplies.  1 (FPX_EINVAL) with badIndex(0) = the first bad offset, malformed message, message of
  // another kind or PreAcceptOk whose dependencies are not n sets in the burst calls' form (parse that one on the JVM);
  // nothing was applied.  badIndex(0) = -1 with status 1: epxLeaderReplies' own refusal
  @native def epxWireLeaderTick(handle: Long, m: Int, numReplicas: Int, in: java.nio.ByteBuffer, inLen: Long,
                                inOffsets: java.nio.ByteBuffer, to: java.nio.ByteBuffer, outcome: Array[Int],
                                triple: Array[Int], outDeps: Array[Int], decided: Array[Int], badIndex: Array[Int]): Int
  // the context's key table (include/fpx.h, fpx_epx_keys_enable): key strings -> key ids on the device (what
  // GpuEPaxosEngine.keyOf is on the JVM), arenaBytes for the strings.  Once per context
  @native def epxKeysEnable(handle: Long, arenaBytes: Long): Int
  // one batch of key strings (fpx_epx_keys_intern): string p = bytes(off(p) until off(p) + len(p)), UTF-8 as on the wire
  // -> ids(p); equal strings get equal ids, new ones the next ids in order of first occurrence.  5 (FPX_ECAPACITY): more
  // keys than numKeys or more bytes than the arena; 1: a key longer than 4096 bytes; nothing applied either way
  @native def epxKeysIntern(handle: Long, count: Int, bytes: Array[Byte], bytesLen: Long, off: Array[Long], len: Array[Int],
                            ids: Array[Int]): Int
  // the context's command store (include/fpx.h, fpx_epx_cmds_enable): triple id -> the serialised CommandOrNoop on the device
  // (what GpuEPaxosEngine.triples is on the JVM), ids below maxTriples, arenaBytes for the bytes.  Once per context.  With it
  // the two ticks below keep the command of every frame under its triple id, and epxWireReplicaTickBytes encodes the Commit sent
  // back and the PrepareOk of a PreAccepted / Accepted instance itself
  @native def epxCmdsEnable(handle: Long, maxTriples: Int, arenaBytes: Long): Int
  // one burst of commands (fpx_epx_cmds_put) for the triple ids that never pass through a tick (the ones handed to epxLead*):
  // command p = bytes(off(p) until off(p) + len(p)) belongs to tripleId(p).  An id that has bytes keeps them; an id >=
  // maxTriples or a command above 65536 bytes is skipped (its replies stay deferred); a burst that does not fit the arena stores
  // nothing.  None of these is an error.  result (4 longs, may be null): new commands, new bytes, skipped, refused (0 / 1)
  @native def epxCmdsPut(handle: Long, count: Int, bytes: Array[Byte], bytesLen: Long, off: Array[Long], len: Array[Int],
                         tripleId: Array[Int], result: Array[Long]): Int
  // out (4 longs): commands stored, arena bytes used, records skipped so far, bursts refused so far
  @native def epxCmdsStats(handle: Long, out: Array[Long]): Int
  // one tick of hosted replicas from wire bytes (include/fpx_wire.h, fpx_wire_epx_replica_tick; needs epxKeysEnable): in /
  // inOffsets / to as epxWireLeaderTick's; PreAccept, Accept, Commit and Prepare frames only.  The triple id of message i is
  // tripleId(i), or with tripleId null tripleBase + i (-1 for a Prepare).  The outputs are epxReplicaInboxMk's.  result(0):
  // -1, or with status 1 the first bad offset, malformed frame, frame of another kind or frame whose dependencies or command
  // are not in the canonical shape (parse that one on the JVM) -- nothing applied, nothing interned; -1 with status 1:
  // epxReplicaInboxMk's own refusal (the burst's keys stay interned).  result(1): the (message, key) pairs; status 5 with
  // more than maxPairs of them (call again), or when the key table is full
  @native def epxWireReplicaTick(handle: Long, m: Int, numReplicas: Int, in: java.nio.ByteBuffer, inLen: Long,
                                 inOffsets: java.nio.ByteBuffer, to: java.nio.ByteBuffer, tripleBase: Int, tripleId: Array[Int],
                                 maxPairs: Int, outcome: Array[Int], reply: Array[Int], outDeps: Array[Int],
                                 result: Array[Int]): Int
  // the same tick, bytes to bytes (fpx_wire_epx_replica_tick_bytes): the replies the replicas send back come out serialised --
  // reply i is out[outOffsets(i) until outOffsets(i + 1)) (direct buffers, native order: outCap bytes, m + 1 longs), empty when
  // replyKind(i) (m bytes) is 0 (nothing to send) or 2 (deferred: a Commit sent back, a PrepareOk that carries a command, a
  // PreAcceptOk of a triple stored by id or with more than 64 explicit ids -- build that one from outcome / reply / outDeps as
  // before).  outcome, reply and outDeps may be null.  result (6 longs): the bad index and the pairs as above, then the replies
  // encoded, the bytes needed, the records deferred and -1.  outCap >= 472 * m (FPX_WIRE_EPX_REPLY_MAX) always suffices
  // without the command store; with it a reply that carries a command of c bytes takes up to 503 + c
  // (FPX_WIRE_EPX_CMD_REPLY_MAX) and only records with by-id dependencies or more than 64 explicit ids stay deferred;
  // status 5 with result(3) > outCap: the tick WAS applied and the arrays are valid -- encode from them
  @native def epxWireReplicaTickBytes(handle: Long, m: Int, numReplicas: Int, in: java.nio.ByteBuffer, inLen: Long,
                                      inOffsets: java.nio.ByteBuffer, to: java.nio.ByteBuffer, tripleBase: Int,
                                      tripleId: Array[Int], maxPairs: Int, out: java.nio.ByteBuffer, outCap: Long,
                                      outOffsets: java.nio.ByteBuffer, replyKind: java.nio.ByteBuffer, outcome: Array[Int],
                                      reply: Array[Int], outDeps: Array[Int], result: Array[Long]): Int
  // one burst of PreAccept (kind 0) / Accept (1) / Commit (2) / Prepare (3) messages from peer replicas, message i to replica
  // to(i), in delivery order, instances repeated freely (handlePreAccept :1159-1289, handleAccept :1421-1511, handleCommit
  // :1567-1575, handlePrepare :1632-1757).  deps (m x n): a row starting with -1 on an Accept / a Commit = the triple is known
  // by its id alone.  outcome (m): 0 ignored, 1 PreAcceptOk, 2 PreAcceptOk again, 3 AcceptOk, 4 AcceptOk again, 5 learnt, 6
  // PrepareOk, 7 Nack, 8 the Commit goes back; reply = ballot (a Nack's largestBallot, a PrepareOk's voteBallot) | PrepareOk
  // status | values end | triple id (4 x m) and outDeps (m x n): the triple of the PreAcceptOk / Commit / PrepareOk to send
  @native def epxReplicaInbox(handle: Long, m: Int, numReplicas: Int, kind: Array[Int], to: Array[Int], leader: Array[Int],
                              number: Array[Int], ballotOrdering: Array[Int], ballotReplica: Array[Int], key: Array[Int],
                              isSet: Array[Byte], tripleId: Array[Int], deps: Array[Int], depsValuesEnd: Array[Int],
                              outcome: Array[Int], reply: Array[Int], outDeps: Array[Int]): Int
  // ---- originating an instance's recovery (include/fpx.h, FPX_EPX_F_RECOVERY): a context with leader state AND the
  // Preparing phase
  @native def epxCreateWithRecovery(numReplicas: Int, numKeys: Int, device: Int, numInstances: Int): Long
  // transitionToPreparePhase at replica at(i) with its own Prepare delivered at once (epaxos/Replica.scala:969-996,
  // 1632-1757).  result (5 x m) = outcome (0 Preparing, 1 the instance is committed here, 2 skipped: fatal in the reference) |
  // the ballot ordering of the Prepare to send | the own PrepareOk's status | voteBallot (encoded) | triple id
  @native def epxRecover(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], at: Array[Int],
                         result: Array[Int]): Int
  // one burst of PrepareOks at hosted replicas, in delivery order (handlePrepareOk :1759-1869).  status 0 NotSeen / 2
  // PreAccepted / 3 Accepted, vote ballot (-1, -1) = null.  outcome (m): 0 ignored, 1 waiting, 2 Accept phase (epxLeadAccept
  // with the triple), 3 pre-accept the command of the triple id again, 4 pre-accept a Noop (both: epxLead, avoidFastPath), 5
  // skipped (fatal in the reference); decision = source | triple id | ballot | sequence number | values end (5 x m) and
  // outDeps (m x n); decided (m + 1): how many decisions, then their indices.  Apply them BEFORE the next burst of any kind
  @native def epxRecoveryReplies(handle: Long, m: Int, numReplicas: Int, to: Array[Int], leader: Array[Int], number: Array[Int],
                                 ballotOrdering: Array[Int], ballotReplica: Array[Int], replicaIndex: Array[Int],
                                 status: Array[Int], voteBallotOrdering: Array[Int], voteBallotReplica: Array[Int],
                                 tripleId: Array[Int], sequenceNumber: Array[Int], deps: Array[Int], depsValuesEnd: Array[Int],
                                 asIntended: Int, outcome: Array[Int], decision: Array[Int], outDeps: Array[Int],
                                 decided: Array[Int]): Int
  // transitionToAcceptPhase at replica at(i) in ballot (ballotOrdering(i), at(i)) with the triple given (:732-793)
  @native def epxLeadAccept(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], at: Array[Int],
                            ballotOrdering: Array[Int], key: Array[Int], isSet: Array[Byte], tripleId: Array[Int],
                            sequenceNumber: Array[Int], deps: Array[Int], depsValuesEnd: Array[Int]): Int
  // the multi-key forms of epxPreaccept / epxAccept / epxHandleCommit / epxHandlePreaccept: command i's keys are
  // keys(keyOffsets(i) until keyOffsets(i + 1)) (keyOffsets: m + 1 entries from 0), everything else as above
  @native def epxPreacceptMk(handle: Long, m: Int, numReplicas: Int, leader: Array[Int],
                             number: Array[Int], keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte],
                             respMask: Array[Byte], seenMask: Array[Byte], rank: Array[Int],
                             fast: Array[Byte], deps: Array[Int], leaderDeps: Array[Int],
                             ownValuesEnd: Array[Int]): Int
  @native def epxAcceptMk(handle: Long, m: Int, leader: Array[Int], number: Array[Int],
                          ballotOrdering: Array[Int], ballotReplica: Array[Int], tripleId: Array[Int],
                          keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte],
                          targetMask: Array[Byte], replies: Array[Byte], nackBallot: Array[Int]): Int
  @native def epxHandleCommitMk(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int],
                                tripleId: Array[Int], keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte],
                                deps: Array[Int], depsValuesEnd: Array[Int], targetMask: Array[Byte]): Int
  @native def epxHandlePreacceptMk(handle: Long, m: Int, numReplicas: Int, leader: Array[Int],
                                   number: Array[Int], ballotOrdering: Array[Int],
                                   ballotReplica: Array[Int], keyOffsets: Array[Int], keys: Array[Int],
                                   isSet: Array[Byte], tripleId: Array[Int], depsIn: Array[Int],
                                   depsInValuesEnd: Array[Int], targetMask: Array[Byte], replies: Array[Byte],
                                   nackBallot: Array[Int], replyDeps: Array[Int], replyEndTriple: Array[Int]): Int
  // ... and of the calls a hosted replica makes among REMOTE peers: epxReplicaInbox, epxLead, epxLeadAccept.  The leader
  // state keeps one key word per instance (the key, -1 for no key, -2 for a list of two or more distinct keys): the
  // caller holds the list by triple id
  @native def epxReplicaInboxMk(handle: Long, m: Int, numReplicas: Int, kind: Array[Int], to: Array[Int], leader: Array[Int],
                                number: Array[Int], ballotOrdering: Array[Int], ballotReplica: Array[Int],
                                keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte], tripleId: Array[Int],
                                deps: Array[Int], depsValuesEnd: Array[Int], outcome: Array[Int], reply: Array[Int],
                                outDeps: Array[Int]): Int
  @native def epxLeadMk(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], at: Array[Int],
                        ballotOrdering: Array[Int], keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte],
                        tripleId: Array[Int], avoidFastPath: Array[Byte], deps: Array[Int], depsValuesEnd: Array[Int]): Int
  @native def epxLeadAcceptMk(handle: Long, m: Int, numReplicas: Int, leader: Array[Int], number: Array[Int], at: Array[Int],
                              ballotOrdering: Array[Int], keyOffsets: Array[Int], keys: Array[Int], isSet: Array[Byte],
                              tripleId: Array[Int], sequenceNumber: Array[Int], deps: Array[Int],
                              depsValuesEnd: Array[Int]): Int
  @native def epxReadCmdlog(handle: Long, numReplicas: Int, replica: Int, leader: Int, number: Int,
                            entry: Array[Int]): Int
  // multi-GPU: one context per GPU, one RCCL communicator over them (fpx_comm_*); the 128-byte id of
  // commUniqueId travels to the other ranks over the actors' own transport
  @native def commUniqueId(id: Array[Byte]): Int
  @native def commCreate(handle: Long, id: Array[Byte], rank: Int, world: Int): Int
  @native def commDestroy(handle: Long): Int
  // wire adapter: a tick of ProxyLeaderInbound byte arrays packed into one direct buffer + n + 1
  // offsets -> fields = kind | slot | round | isNoop | valueLen | groupIndex | acceptorIndex (7 x n)
  @native def wireDecodeProxyLeaderInbound(buf: java.nio.ByteBuffer, offsets: Array[Long], n: Int,
                                           fields: Array[Int], valueOff: Array[Long],
                                           badIndex: Array[Int]): Int
  // the acceptors' half of Phase 1 and the log window (fpx_acceptor_phase1b_info, fpx_read_acceptor,
  // fpx_recycle_slots, fpx_proxy_forget)
  @native def acceptorPhase1bInfo(handle: Long, group: Int, replica: Int, chosenWatermark: Int, cap: Int,
                                  slot: Array[Int], voteRound: Array[Int], voteValue: Array[Int]): Int // count, < 0: -status
  // a Leader's Phase1a at every acceptor it addresses in ONE call (fpx_acceptor_phase1): targetMasks 4 x numGroups words
  // (null: everybody), bits = promised | nack (4 x numGroups words each), entry group * perGroup + replica owns
  // offsets(e) until offsets(e + 1) of the record arrays (empty unless it promised); count, < 0: -status
  @native def acceptorPhase1All(handle: Long, round: Int, chosenWatermark: Int, numGroups: Int, targetMasks: Array[Long],
                                bits: Array[Long], cap: Int, offsets: Array[Long], slot: Array[Int],
                                voteRound: Array[Int], voteValue: Array[Int]): Long
  // Leader.handlePhase1b for a burst of Phase1bs in delivery order (fpx_leader_phase1b_msgs): scalars = (round,
  // chosenWatermark, leaderGroup, recoverSlot, flags, gridCols); message i owns the records offsets(i) until
  // offsets(i + 1); result = 8 longs (complete, decidedAt, count, maxSlot, nextSlot, written), -1 where nothing was written
  @native def leaderPhase1bMsgs(handle: Long, scalars: Array[Int], n: Int, kind: Array[Int], msgRound: Array[Int],
                                groupIndex: Array[Int], acceptorIndex: Array[Int], offsets: Array[Long],
                                infoSlot: Array[Int], infoVoteRound: Array[Int], infoValue: Array[Int], cap: Int,
                                outSlot: Array[Int], safeRound: Array[Int], safeValue: Array[Int], result: Array[Long],
                                heldBits: Array[Long]): Int
  @native def acceptorRound(handle: Long, group: Int, replica: Int): Int // Acceptor.round, < -1: -status - 1
  // the largest row of [firstRow, firstRow + count) in which the acceptor holds a vote, -1: none, < -1: -status - 1
  @native def acceptorMaxVotedIn(handle: Long, group: Int, replica: Int, firstRow: Int, count: Int): Int
  @native def recycleSlots(handle: Long, firstSlot: Int, count: Int): Int
  @native def proxyForget(handle: Long, firstSlot: Int, count: Int): Int
  // wire adapter, acceptor side: AcceptorInbound bytes -> fields = kind | slot | round | isNoop | valueLen |
  // chosenWatermark (6 x n); LeaderInbound{Phase1b} / {Nack} bytes into a direct buffer (length, < 0: -needed)
  @native def wireDecodeAcceptorInbound(buf: java.nio.ByteBuffer, offsets: Array[Long], n: Int,
                                        fields: Array[Int], valueOff: Array[Long], badIndex: Array[Int]): Int
  @native def wireEncodeLeaderPhase1b(out: java.nio.ByteBuffer, groupIndex: Int, acceptorIndex: Int, round: Int,
                                      nInfo: Int, slot: Array[Int], voteRound: Array[Int],
                                      values: java.nio.ByteBuffer, valueOff: Array[Long], valueLen: Array[Int],
                                      isNoop: Array[Byte]): Long
  @native def wireEncodeLeaderNack(out: java.nio.ByteBuffer, round: Int): Long
  // Mencius on the wire (mencius/Mencius.proto): ProxyLeaderInbound -> fields = kind | slot | slotEnd | round | isNoop |
  // valueLen | groupIndex | acceptorIndex (8 x n); AcceptorInbound -> kind | slot | slotEnd | round | isNoop | valueLen |
  // chosenWatermark (7 x n); LeaderInbound{Nack} is field 7 there.  Phase1b has MultiPaxos' layout: wireEncodeLeaderPhase1b
  @native def wireMenciusDecodeProxyLeaderInbound(buf: java.nio.ByteBuffer, offsets: Array[Long], n: Int,
                                                  fields: Array[Int], valueOff: Array[Long],
                                                  badIndex: Array[Int]): Int
  @native def wireMenciusDecodeAcceptorInbound(buf: java.nio.ByteBuffer, offsets: Array[Long], n: Int,
                                               fields: Array[Int], valueOff: Array[Long], badIndex: Array[Int]): Int
  @native def wireMenciusEncodeLeaderNack(out: java.nio.ByteBuffer, round: Int): Long
  // EPaxos on the wire (epaxos/EPaxos.proto ReplicaInbound): fields = kind | instanceLeader | instanceNumber |
  // ballotOrdering | ballotReplica | replicaIndex | sequenceNumber | voteBallotOrdering | voteBallotReplica | status |
  // isNoop | cmdLen | depsNumReplicas (13 x n); explicit ids of message i: values[valuesOff(i) .. valuesOff(i + 1))
  // (leaders) and the same range behind valuesCap (ids)
  @native def wireEpaxosDecodeReplicaInbound(buf: java.nio.ByteBuffer, offsets: Array[Long], n: Int, maxReplicas: Int,
                                             fields: Array[Int], cmdOff: Array[Long], depsWatermark: Array[Int],
                                             valuesOff: Array[Long], valuesCap: Int, values: Array[Int],
                                             badIndex: Array[Int]): Int
  // head = kind | instanceLeader | instanceNumber | ballotOrdering | ballotReplica | replicaIndex | sequenceNumber |
  // voteBallotOrdering | voteBallotReplica | status | isNoop (11 ints)
  @native def wireEpaxosEncodeReplicaInbound(out: java.nio.ByteBuffer, head: Array[Int], command: java.nio.ByteBuffer,
                                             commandOff: Long, commandLen: Int, numReplicas: Int,
                                             depsWatermark: Array[Int], numValues: Int, values: Array[Int]): Long

  def check(status: Int, logger: Logger): Unit = status match {
    case OK                       => ()
    case EINVAL                   => throw new IllegalArgumentException("libfpx: require failed")
    case EFATAL_UNKNOWN_SLOTROUND =>
      logger.fatal("A ProxyLeader received a Phase2b in a slot and round it never sent a Phase2a in.")
    case s => logger.fatal(s"libfpx status $s")
  }
}

// One libfpx context = the acceptors of every group + the proxy leader's tallies, for a deployment whose
// acceptors and proxy leaders run in ONE process on the GPU box (one Transport event loop: the engine is
// not thread-safe, like every actor, Transport.scala:37-39).
//
// The log window.  The context holds `numSlots` rows; slot s lives in row s % numSlots, the window is
// [base, base + numSlots).  A Phase2a beyond the window waits (`deferred`) until the window has moved; the
// window moves, in chunks, over slots that (a) were chosen through this engine -- Chosen was sent to every
// replica -- and (b) lie at least `retain` slots behind the highest chosen slot: their rows are recycled
// (votes dropped, tallies forgotten, the JVM-side value bytes released).  The reference's acceptors and proxy
// leaders never forget anything (Acceptor.scala:98, ProxyLeader.scala:135); the deviation this buys bounded
// memory with: a replica that lost a Chosen more than `retain` slots ago can no longer recover it from these
// acceptors, so `retain` bounds how far a replica may lag.
class GpuPhase2Engine[Transport <: frankenpaxos.Transport[Transport]](
    logger: Logger,
    config: Config[Transport],
    numSlots: Int = 1 << 20,
    retainSlots: Int = 1 << 18,
    // thrifty delivery (the reference's default, ProxyLeader.scala:190-191: every Phase2a goes to f + 1 of its group's
    // 2f + 1 acceptors).  The reference shuffles; any f + 1 will do, and this engine sends to a window of f + 1
    // NEIGHBOURING acceptors that rotates from message to message -- see thriftyMask
    thrifty: Boolean = true
) {
  config.checkValid()
  val perGroup: Int = config.acceptorAddresses(0).size
  val numGroups: Int = config.numAcceptorGroups
  // rows keep their acceptor group when the log wraps (slot % numGroups == row % numGroups)
  logger.check(config.flexible || numSlots % numGroups == 0)
  private val chunk = math.max(1, numSlots / 16)
  logger.check(retainSlots + 2 * chunk <= numSlots)

  private val cfg: Array[Int] =
    if (!config.flexible)
      Array(numSlots, perGroup, numGroups, 1, config.f, /*THRESHOLD*/ 0, 0, 0,
            config.numLeaders, /*ACCEPTOR*/ 0, 4, 0, 0, 0, 0)
    else
      Array(numSlots, numGroups * perGroup, 1, 1, config.f, /*GRID*/ 2,
            numGroups, perGroup, config.numLeaders, 0, 4, 0, 0, 0, 0)
  private val handle = Native.create(cfg)
  if (handle < 0) Native.check((-handle).toInt, logger)

  // where acceptor (groupIndex, index) of the reference's addressing lives in the context
  def ctxGroup(groupIndex: Int): Int = if (config.flexible) 0 else groupIndex
  def ctxReplica(groupIndex: Int, index: Int): Int = if (config.flexible) groupIndex * perGroup + index else index

  // ---- value ids: the int32 the GPU carries stands for a CommandBatchOrNoop kept here; Noop is FPX_NOOP = -1.
  // An id lives as long as the row it was proposed in: votes and tallies of the row are its only holders.
  private val values = mutable.ArrayBuffer[CommandBatchOrNoop]()
  private val freeIds = mutable.ArrayStack[Int]()
  private val idsOfRow = Array.fill(numSlots)(List.empty[Int])
  private def intern(row: Int, v: CommandBatchOrNoop): Int =
    if (v.value.isNoop) -1
    else {
      val id = if (freeIds.nonEmpty) freeIds.pop() else { values += null; values.size - 1 }
      values(id) = v
      idsOfRow(row) = id :: idsOfRow(row)
      id
    }
  def valueOf(id: Int): CommandBatchOrNoop =
    if (id < 0) CommandBatchOrNoop().withNoop(Noop()) else values(id)

  // ---- the window
  private var base = 0                                   // first slot of the window (a multiple of chunk)
  private val chosenInWindow = new java.util.BitSet(numSlots) // by row
  private var chosenPrefix = 0                           // every slot in [base, chosenPrefix) is chosen
  private var highestChosen = -1
  private val deferred = mutable.Queue[Phase2a]()
  private def row(slot: Int): Int = slot % numSlots
  private def slotOfRow(r: Int): Int = base + ((r - row(base)) % numSlots + numSlots) % numSlots

  private def markChosen(slot: Int): Unit = {
    chosenInWindow.set(row(slot))
    highestChosen = math.max(highestChosen, slot)
    while (chosenPrefix < base + numSlots && chosenInWindow.get(row(chosenPrefix))) chosenPrefix += 1
  }
  // moves the window over chosen slots that are old enough; true if it moved
  private def advanceWindow(): Boolean = {
    var moved = false
    while (chosenPrefix - base >= chunk && highestChosen - (base + chunk) >= retainSlots) {
      val r0 = row(base)                                 // chunk | numSlots: the chunk does not wrap
      refreshStaleGroups()                               // (the votes of these rows are read before they are cleared)
      Native.check(Native.recycleSlots(handle, r0, chunk), logger)
      for (r <- r0 until r0 + chunk) {
        idsOfRow(r).foreach(id => { values(id) = null; freeIds.push(id) })
        idsOfRow(r) = Nil
        chosenInWindow.clear(r)
      }
      base += chunk
      moved = true
    }
    moved
  }

  // ---- the read path: Acceptor.maxVotedSlot (multipaxos/Acceptor.scala:104, 208) of every acceptor, in SLOTS.  The
  // device keeps the scalar over rows, which stops being the maximum over slots once the window has wrapped; so the
  // engine follows it here.  A message nobody Nacked was voted for by every acceptor it went to (Acceptor.scala:201-219):
  // the tick's outputs say that much without any per-acceptor answer.  After a tick with a Nack the engine does not know
  // which of the message's acceptors voted; the group is marked stale and the next read asks the device for the largest
  // voted row of each lap of the window (fpx_acceptor_max_voted_in) -- exact again, and only after leader changes.
  private val ctxGroups = if (config.flexible) 1 else numGroups
  private val ctxReplicas = if (config.flexible) numGroups * perGroup else perGroup
  private val maxVoted = Array.fill(ctxGroups, ctxReplicas)(-1)
  private val maxVotedStale = Array.fill(ctxGroups)(false)
  private def groupOfSlot(slot: Int): Int = if (config.flexible) 0 else slot % numGroups

  // after a tick: `slot` = the messages' slots (log positions, not rows), masks = their targets (null: everyone)
  private def noteVotes(slots: Array[Int], nackRound: Array[Int], masks: Array[Long]): Unit = {
    // descending by slot: an acceptor's maximum is the first Nack-free message that reached it
    val order = slots.indices.sortBy(i => -slots(i).toLong)
    val covered = Array.fill(ctxGroups)(new java.util.BitSet(ctxReplicas))
    for (i <- order) {
      val g = groupOfSlot(slots(i))
      if (nackRound(i) >= 0) maxVotedStale(g) = true
      else if (covered(g).cardinality < ctxReplicas) {
        for (a <- 0 until ctxReplicas
             if !covered(g).get(a) && (masks == null || (masks(4 * i + (a >> 6)) & (1L << (a & 63))) != 0)) {
          covered(g).set(a)
          maxVoted(g)(a) = math.max(maxVoted(g)(a), slots(i))
        }
      }
    }
  }

  // the rescan of one stale group: the largest voted row of each lap of the window, per acceptor, from the device
  private def refreshMaxVoted(g: Int): Unit = {
    val r0 = row(base)
    for (b <- 0 until ctxReplicas) {
      // the older lap of the window lives in rows [r0, numSlots), the newer one in [0, r0)
      val hi = if (r0 > 0) Native.acceptorMaxVotedIn(handle, g, b, 0, r0) else -1
      val lo = if (hi < 0) Native.acceptorMaxVotedIn(handle, g, b, r0, numSlots - r0) else -1
      if (hi < -1) Native.check(-hi - 1, logger)
      if (lo < -1) Native.check(-lo - 1, logger)
      val slot = if (hi >= 0) base + (numSlots - r0) + hi else if (lo >= 0) base + (lo - r0) else -1
      maxVoted(g)(b) = math.max(maxVoted(g)(b), slot)
    }
    maxVotedStale(g) = false
  }
  // ADVICE r05: a stale group is rescanned BEFORE any of its rows is recycled (advanceWindow) -- a vote cast in a Nacked
  // message must be recorded before its row is cleared, or MaxSlotReply.slot would under-report (Acceptor.scala:208 never
  // misses a vote, and a low slot is the unsafe direction for linearizable reads)
  private def refreshStaleGroups(): Unit =
    for (g <- 0 until ctxGroups if maxVotedStale(g)) refreshMaxVoted(g)

  // Acceptor.handleMaxSlotRequest / handleBatchMaxSlotRequest reply with this (Acceptor.scala:222-254)
  def maxVotedSlot(groupIndex: Int, index: Int): Int = {
    val g = ctxGroup(groupIndex); val a = ctxReplica(groupIndex, index)
    if (maxVotedStale(g)) refreshMaxVoted(g)
    maxVoted(g)(a)
  }

  // ---- which acceptors a Phase2a goes to.  A window of f + 1 neighbouring acceptors: on groups of 253 .. 256 acceptors it
  // moves in steps of 16 (a 64-byte sector of the group's row in HBM) and does not wrap over the end of the row -- the
  // runs libfpx walks two rows per wavefront step (include/fpx.h, FPX_F_SCATTERED_TARGETS); on the small groups of an
  // everyday deployment it moves by one acceptor and wraps, so every acceptor sees (f + 1) / (2f + 1) of the messages
  private var rotor = 0
  private def thriftyMask(masks: Array[Long], at: Int): Unit = {
    val q = config.f + 1
    val start = if (perGroup >= 253) 16 * (rotor % ((perGroup - q) / 16 + 1)) else rotor % perGroup
    rotor += 1
    for (j <- 0 until q) {
      val a = (start + j) % perGroup
      masks(4 * at + (a >> 6)) |= 1L << (a & 63)
    }
  }

  // ---- Phase 2: one tick of Phase2a messages (ProxyLeader.handlePhase2a + every Acceptor.handlePhase2a +
  // ProxyLeader.handlePhase2b).  Returns, in message order, Chosen to broadcast and (round, Nack) to route.
  case class TickResult(chosen: Seq[Chosen], nacks: Seq[(Int, Nack)])
  def phase2Tick(incoming: Seq[Phase2a]): TickResult = {
    val chosenOut = mutable.Buffer[Chosen](); val nackOut = mutable.Buffer[(Int, Nack)]()
    var batch: Seq[Phase2a] = deferred.dequeueAll(_ => true) ++ incoming
    while (batch.nonEmpty) {
      // below the window: chosen long ago and recycled -- nothing left to vote on; beyond it: wait
      val (now, later) = batch.filter(_.slot >= base).partition(_.slot < base + numSlots)
      val n = now.size
      val slot = new Array[Int](n); val round = new Array[Int](n); val value = new Array[Int](n)
      for ((p, i) <- now.zipWithIndex) {
        slot(i) = row(p.slot); round(i) = p.round; value(i) = intern(row(p.slot), p.commandBatchOrNoop)
      }
      val chosen = new Array[Byte](n); val cr = new Array[Int](n); val cv = new Array[Int](n)
      val nr = new Array[Int](n)
      // thrifty: one mask of f + 1 acceptors per message (ProxyLeader.scala:190-191); a flexible deployment's grid
      // column (:193-196) is not generated here: dense delivery (targetMask = null), as without `thrifty`
      val masks: Array[Long] =
        if (thrifty && !config.flexible && perGroup > config.f + 1) {
          val m = new Array[Long](4 * n)
          for (i <- 0 until n) thriftyMask(m, i)
          m
        } else null
      if (n > 0) Native.check(Native.phase2Fused(handle, n, slot, round, value, masks, chosen, cr, cv, nr), logger)
      noteVotes(now.map(_.slot).toArray, nr, masks)
      for (i <- 0 until n) {
        if (chosen(i) != 0) {
          chosenOut += Chosen(slot = now(i).slot, commandBatchOrNoop = valueOf(cv(i))) // ProxyLeader.scala:246-253
          markChosen(now(i).slot)
        }
        // Acceptor.scala:197-198: Nack(round = acceptor's round) to leaders(roundSystem.leader(phase2a.round))
        if (nr(i) >= 0) nackOut += ((round(i), Nack(round = nr(i))))
      }
      // a moved window may admit what waited; otherwise it keeps waiting for the slots before it to be chosen
      batch = if (advanceWindow()) later else { deferred ++= later; Seq.empty }
    }
    TickResult(chosenOut, nackOut)
  }

  // ---- Phase 2 among REMOTE (reference) acceptors: the engine keeps the proxy leader's tallies only.
  // ProxyLeader.handlePhase2a's bookkeeping for one tick (ProxyLeader.scala:175-184, 213): opens the tallies and returns
  // the Phase2as that were new, in message order -- the caller forwards exactly those to the acceptors (:186-211); a
  // duplicate is not forwarded.  The window is kept as in phase2Tick: what lies beyond it waits, what lies below it
  // was chosen long ago.
  def openPhase2as(incoming: Seq[Phase2a]): Seq[Phase2a] = {
    val fresh = mutable.Buffer[Phase2a]()
    val batch: Seq[Phase2a] = deferred.dequeueAll(_ => true) ++ incoming
    val (now, later) = batch.filter(_.slot >= base).partition(_.slot < base + numSlots)
    deferred ++= later
    val n = now.size
    val slot = new Array[Int](n); val round = new Array[Int](n); val value = new Array[Int](n)
    for ((p, i) <- now.zipWithIndex) {
      slot(i) = row(p.slot); round(i) = p.round; value(i) = intern(row(p.slot), p.commandBatchOrNoop)
    }
    val isNew = new Array[Byte](n)
    if (n > 0) Native.check(Native.proxyOpen(handle, n, slot, round, value, isNew), logger)
    for (i <- 0 until n if isNew(i) != 0) fresh += now(i)
    fresh
  }

  // ProxyLeader.handlePhase2b for one tick of Phase2bs from remote acceptors (ProxyLeader.scala:217-258), tallied on the
  // device in ONE native call (fpx_proxy_phase2b_msgs).  Returns the Chosen to broadcast, in message order; the window,
  // row and markChosen bookkeeping is phase2Tick's.  A Phase2b below the window answers a slot chosen and recycled
  // long ago (the reference's `Done`: ignored); one beyond it was never opened here.
  def tallyPhase2bs(msgs: Seq[Phase2b]): Seq[Chosen] = {
    val chosenOut = mutable.Buffer[Chosen]()
    val now = msgs.filter(m => m.slot >= base && m.slot < base + numSlots)
    val n = now.size
    if (n == 0) return chosenOut
    val group = new Array[Int](n); val acc = new Array[Int](n); val slot = new Array[Int](n); val round = new Array[Int](n)
    for ((m, i) <- now.zipWithIndex) {
      group(i) = m.groupIndex; acc(i) = m.acceptorIndex; slot(i) = row(m.slot); round(i) = m.round
    }
    val chosen = new Array[Byte](n); val cr = new Array[Int](n); val cv = new Array[Int](n)
    // a grid's bit is groupIndex * perGroup + acceptorIndex (ctxReplica); otherwise the group follows from the slot
    val gridCols = if (config.flexible) perGroup else 0
    Native.check(Native.proxyPhase2bMsgs(handle, n, null, group, acc, slot, round, gridCols, chosen, cr, cv), logger)
    for (i <- 0 until n if chosen(i) != 0) {
      chosenOut += Chosen(slot = now(i).slot, commandBatchOrNoop = valueOf(cv(i))) // ProxyLeader.scala:246-253
      markChosen(now(i).slot)
    }
    advanceWindow()                                      // what it admits is opened by the next openPhase2as
    chosenOut
  }

  // ---- Phase 1, acceptor side (Acceptor.handlePhase1a, multipaxos/Acceptor.scala:148-182)
  def handlePhase1a(groupIndex: Int, index: Int, phase1a: Phase1a): Either[Nack, Phase1b] = {
    val g = ctxGroup(groupIndex); val a = ctxReplica(groupIndex, index)
    val target = new Array[Long](4); target(a >> 6) = 1L << (a & 63)
    val bits = new Array[Long](8)
    // rows, not slots: a watermark inside the window is a row boundary only when the window does not wrap
    // between it and the window's end -- promise from row 0 on (more than asked for is safe, Acceptor.scala
    // promises on its single `round` anyway) and filter the info by slot below
    Native.check(Native.acceptorPhase1a(handle, g, phase1a.round, 0, target, bits), logger)
    if ((bits(4 + (a >> 6)) & (1L << (a & 63))) != 0) {
      // :155-162  phase1a.round < round: Nack(round)
      return Left(Nack(round = Native.acceptorRound(handle, g, a)))
    }
    // :163-181  Phase1b(info = votes in slots >= chosenWatermark, ascending)
    Right(Phase1b(groupIndex = groupIndex, acceptorIndex = index, round = phase1a.round,
                  info = phase1bInfo(g, a, phase1a.chosenWatermark)))
  }

  // Phase1b.info of one acceptor: its votes in slots >= chosenWatermark, ascending (Acceptor.scala:167-180)
  private def phase1bInfo(g: Int, a: Int, chosenWatermark: Int): Seq[Phase1bSlotInfo] = {
    var cap = 1024
    var slots = new Array[Int](cap); var vr = new Array[Int](cap); var vv = new Array[Int](cap)
    var k = Native.acceptorPhase1bInfo(handle, g, a, 0, cap, slots, vr, vv)
    if (k > cap) {
      cap = k; slots = new Array[Int](cap); vr = new Array[Int](cap); vv = new Array[Int](cap)
      k = Native.acceptorPhase1bInfo(handle, g, a, 0, cap, slots, vr, vv)
    }
    if (k < 0) Native.check(-k, logger)
    (0 until k)
      .map(j => Phase1bSlotInfo(slot = slotOfRow(slots(j)), voteRound = vr(j), voteValue = valueOf(vv(j))))
      .filter(_.slot >= chosenWatermark)
      .sortBy(_.slot)
  }

  // ---- Phase 1 for a run of Phase1as of ONE round: a new leader sends one to every acceptor address, and they arrive
  // together (inboxBurst below hands them over).  ONE native call per run (fpx_acceptor_phase1: the round movement of every
  // addressed group, then the Phase1b.info of exactly the promisers, compacted on the device), each acceptor answered from
  // its slice.  As in handlePhase1a the call runs with watermark row 0; the per-slot filter and slotOfRow stay here.
  private def phase1Run(run: List[(Int, Int, Phase1a, Either[Nack, Phase1b] => Unit)]): Unit = {
    val phase1a = run.head._3
    val words = 4 * ctxGroups
    val target = new Array[Long](words)
    for ((g, i, _, _) <- run) {
      val a = ctxReplica(g, i)
      target(4 * ctxGroup(g) + (a >> 6)) |= 1L << (a & 63)
    }
    val bits = new Array[Long](2 * words)
    val offsets = new Array[Long](ctxGroups * ctxReplicas + 1)
    var cap = 1024 * run.size
    var slots = new Array[Int](cap); var vr = new Array[Int](cap); var vv = new Array[Int](cap)
    var k = Native.acceptorPhase1All(handle, phase1a.round, 0, ctxGroups, target, bits, cap, offsets, slots, vr, vv)
    if (k > cap) {
      // the promises hold; the same call again answers the same (a promiser promises its own round again)
      cap = k.toInt; slots = new Array[Int](cap); vr = new Array[Int](cap); vv = new Array[Int](cap)
      k = Native.acceptorPhase1All(handle, phase1a.round, 0, ctxGroups, target, bits, cap, offsets, slots, vr, vv)
    }
    if (k < 0) Native.check((-k).toInt, logger)
    for ((g, i, p, reply) <- run) {
      val cg = ctxGroup(g); val a = ctxReplica(g, i)
      if ((bits(words + 4 * cg + (a >> 6)) & (1L << (a & 63))) != 0) {
        reply(Left(Nack(round = Native.acceptorRound(handle, cg, a))))                  // Acceptor.scala:155-162
      } else {
        val e = cg * ctxReplicas + a
        val info = (offsets(e).toInt until offsets(e + 1).toInt)                        // Acceptor.scala:163-181
          .map(j => Phase1bSlotInfo(slot = slotOfRow(slots(j)), voteRound = vr(j), voteValue = valueOf(vv(j))))
          .filter(_.slot >= p.chosenWatermark)
          .sortBy(_.slot)
        reply(Right(Phase1b(groupIndex = g, acceptorIndex = i, round = p.round, info = info)))
      }
    }
  }

  // ---- the acceptors' inbox as a burst (fpx_acceptor_inbox).  Among reference proxy leaders every Phase2a arrives once per
  // acceptor address, f + 1 times per slot (ProxyLeader.scala:190-215), with the clients' and read batchers' reads and now
  // and then a leader's Phase1as between them.  The GpuAcceptors enqueue whatever they receive here; the zero-delay timer
  // of the first message flushes the queue: ONE native call per burst, every acceptor answered from its message's reply,
  // exactly as if each had handled its messages one by one.  The call does not produce Phase1b.info -- a promise's info is
  // the acceptor's votes as of that message -- so a burst is cut after each maximal run of Phase1as, and the promisers of
  // that run get their info from acceptorPhase1All's slices (no vote lies between the promise and the end of the burst).
  sealed trait InboxReply
  case class Voted(phase2b: Phase2b) extends InboxReply
  case class Nacked(nack: Nack) extends InboxReply
  case class Promised(phase1b: Phase1b) extends InboxReply
  case class MaxVotedSlot(slot: Int) extends InboxReply
  private case class InboxMsg(groupIndex: Int, index: Int, request: AcceptorInbound.Request, reply: InboxReply => Unit) {
    def isPhase1a: Boolean = request.isPhase1A
  }
  private val pendingInbox = mutable.Buffer[InboxMsg]()

  // true: the queue was empty -- the caller starts its tick
  def enqueueInbox(groupIndex: Int, index: Int, request: AcceptorInbound.Request, reply: InboxReply => Unit): Boolean = {
    val first = pendingInbox.isEmpty
    pendingInbox += InboxMsg(groupIndex, index, request, reply)
    first
  }

  def flushInbox(): Unit = {
    var rest = pendingInbox.toList
    pendingInbox.clear()
    while (rest.nonEmpty) {
      val (head, tail) = rest.span(!_.isPhase1a)
      val (phase1as, later) = tail.span(_.isPhase1a)
      rest = later
      val burst = head ++ phase1as
      if (burst.size == 1) loneInboxMsg(burst.head) else inboxBurst(burst, head.size)
    }
  }

  private def loneInboxMsg(m: InboxMsg): Unit = m.request match {
    case AcceptorInbound.Request.Phase2A(p) =>
      m.reply(handlePhase2a(m.groupIndex, m.index, p).fold(Nacked(_), Voted(_)))
    case AcceptorInbound.Request.Phase1A(p) =>
      m.reply(handlePhase1a(m.groupIndex, m.index, p).fold(Nacked(_), Promised(_)))
    case _ => m.reply(MaxVotedSlot(maxVotedSlot(m.groupIndex, m.index)))
  }

  // burst = any messages but Phase1as, then (from firstPhase1a on) a run of Phase1as
  private def inboxBurst(burst: List[InboxMsg], firstPhase1a: Int): Unit = {
    val n = burst.size
    val kind = new Array[Int](n); val group = new Array[Int](n); val acc = new Array[Int](n)
    val slot = Array.fill(n)(-1); val round = Array.fill(n)(-1); val value = Array.fill(n)(-1)
    refreshStaleGroups()                                 // maxVoted is followed from the replies below: exact before the burst
    for ((m, i) <- burst.zipWithIndex) {
      // the context's addressing: a grid is ONE group of numGroups x perGroup, bit = groupIndex * perGroup + index
      group(i) = m.groupIndex; acc(i) = m.index
      m.request match {
        case AcceptorInbound.Request.Phase2A(p) =>
          logger.check(p.slot >= base && p.slot < base + numSlots)
          kind(i) = Native.WIRE_PHASE2A; slot(i) = row(p.slot); round(i) = p.round
          value(i) = intern(row(p.slot), p.commandBatchOrNoop)
        case AcceptorInbound.Request.Phase1A(p) => kind(i) = Native.WIRE_PHASE1A; round(i) = p.round
        case AcceptorInbound.Request.MaxSlotRequest(_) => kind(i) = Native.WIRE_MAX_SLOT_REQUEST
        case AcceptorInbound.Request.BatchMaxSlotRequest(_) => kind(i) = Native.WIRE_BATCH_MAX_SLOT_REQUEST
        case AcceptorInbound.Request.Empty => logger.fatal("Empty AcceptorInbound encountered.")
      }
    }
    val replyKind = new Array[Int](n); val replyValue = new Array[Int](n)
    val gridCols = if (config.flexible) perGroup else 0
    Native.check(Native.acceptorInbox(handle, n, kind, group, acc, slot, round, value, gridCols, replyKind, replyValue),
                 logger)
    // everything but the promises, in delivery order.  Acceptor.maxVotedSlot in SLOTS is followed here, vote by vote (the
    // device's scalar is over rows, and the lap query is for votes the engine did not see one by one)
    for ((m, i) <- burst.zipWithIndex) {
      val g = ctxGroup(m.groupIndex); val a = ctxReplica(m.groupIndex, m.index)
      (m.request, replyKind(i)) match {
        case (_, Native.WIRE_NACK) => m.reply(Nacked(Nack(round = replyValue(i))))          // Acceptor.scala:155-162, 192-199
        case (AcceptorInbound.Request.Phase2A(p), _) =>                                     // Acceptor.scala:204-219
          maxVoted(g)(a) = math.max(maxVoted(g)(a), p.slot)
          m.reply(Voted(Phase2b(groupIndex = m.groupIndex, acceptorIndex = m.index, slot = p.slot, round = p.round)))
        case (AcceptorInbound.Request.Phase1A(_), _) => ()                                  // below
        case _ => m.reply(MaxVotedSlot(maxVoted(g)(a)))                                     // Acceptor.scala:222-254
      }
    }
    // the promisers of the run of Phase1as.  An acceptor's round after the run is its last promise's; the promises of
    // that round are fetched per round by acceptorPhase1All (promising an equal round again changes nothing, :155), an
    // earlier promise of an acceptor that promised twice in one run by acceptorPhase1bInfo -- the votes are the same
    val promisers = burst.zipWithIndex.drop(firstPhase1a).filter(mi => replyKind(mi._2) == Native.WIRE_PHASE1B).map(_._1)
    val lastRound = mutable.Map[(Int, Int), Int]()
    for (m <- promisers) lastRound((m.groupIndex, m.index)) = m.request.phase1A.get.round
    val (current, earlier) = promisers.partition(m => lastRound((m.groupIndex, m.index)) == m.request.phase1A.get.round)
    for ((_, run) <- current.groupBy(_.request.phase1A.get.round).toSeq.sortBy(_._1))
      phase1Run(run.map(m => (m.groupIndex, m.index, m.request.phase1A.get, (r: Either[Nack, Phase1b]) =>
        m.reply(r.fold(Nacked(_), Promised(_))))))
    for (m <- earlier) {
      val p = m.request.phase1A.get
      m.reply(Promised(Phase1b(groupIndex = m.groupIndex, acceptorIndex = m.index, round = p.round,
                               info = phase1bInfo(ctxGroup(m.groupIndex), ctxReplica(m.groupIndex, m.index), p.chosenWatermark))))
    }
  }

  // ONE Phase2a at one acceptor, for a message that arrives alone (a burst goes through inboxBurst):
  // Acceptor.handlePhase2a, multipaxos/Acceptor.scala:184-220
  def handlePhase2a(groupIndex: Int, index: Int, p: Phase2a): Either[Nack, Phase2b] = {
    logger.check(p.slot >= base && p.slot < base + numSlots)
    val a = ctxReplica(groupIndex, index)
    val target = new Array[Long](4); target(a >> 6) = 1L << (a & 63)
    val votes = new Array[Long](4); val nacks = new Array[Long](4); val nr = new Array[Int](1)
    Native.check(Native.acceptorPhase2a(handle, 1, Array(row(p.slot)), Array(p.round),
                                        Array(intern(row(p.slot), p.commandBatchOrNoop)), target, votes, nacks, nr),
                 logger)
    if (nr(0) >= 0) Left(Nack(round = nr(0)))
    else {
      val g = ctxGroup(groupIndex)
      maxVoted(g)(a) = math.max(maxVoted(g)(a), p.slot)                               // Acceptor.scala:208
      Right(Phase2b(groupIndex = groupIndex, acceptorIndex = index, slot = p.slot, round = p.round))
    }
  }

  def close(): Unit = Native.check(Native.destroy(handle), logger)
}

// ---- Phase 1, leader side: a leader among acceptors that are NOT in its context (reference Acceptor actors, the
// shards of a replica-sharded group).  The Phase1bs are appended as they arrive and the whole burst is handed to
// fpx_leader_phase1b_msgs, which is stateless and decides exactly where Leader.handlePhase1b would have
// (multipaxos/Leader.scala:504-577): call again with the longer burst until it is complete.  `handle` is any context
// with the deployment's geometry (groups, f, the grid); value ids are positions in `values`, -1 = Noop.
class GpuLeaderRecoveryCore(logger: Logger, handle: Long, round: Int, chosenWatermark: Int, leaderGroup: Int,
                            recoverSlot: Int, gridCols: Int, flags: Int) {
  private val msgRound = mutable.ArrayBuffer[Int](); private val group = mutable.ArrayBuffer[Int]()
  private val acc = mutable.ArrayBuffer[Int](); private val offsets = mutable.ArrayBuffer[Long](0L)
  private val slot = mutable.ArrayBuffer[Int](); private val voteRound = mutable.ArrayBuffer[Int]()
  private val valueId = mutable.ArrayBuffer[Int]()
  // (outSlot, safeValueId) per re-proposed slot, nextSlot
  case class Recovered(slots: Array[Int], valueIds: Array[Int], nextSlot: Int)

  def append(r: Int, groupIndex: Int, acceptorIndex: Int, info: Seq[(Int, Int, Int)]): Unit = {
    msgRound += r; group += groupIndex; acc += acceptorIndex
    for ((s, vr, id) <- info) { slot += s; voteRound += vr; valueId += id }
    offsets += slot.size.toLong
  }

  // None: still waiting for a quorum
  def tryRecover(): Option[Recovered] = {
    val scalars = Array(round, chosenWatermark, leaderGroup, recoverSlot, flags, gridCols)
    val n = msgRound.size
    val (mr, g, a, off) = (msgRound.toArray, group.toArray, acc.toArray, offsets.toArray)
    val (s, vr, id) = (slot.toArray, voteRound.toArray, valueId.toArray)
    val result = new Array[Long](8)
    def call(cap: Int, os: Array[Int], sr: Array[Int], sv: Array[Int]): Unit = {
      val st = Native.leaderPhase1bMsgs(handle, scalars, n, null, mr, g, a, off, s, vr, id, cap, os, sr, sv, result, null)
      if (st != 0 && st != 5 /*FPX_ECAPACITY: the sizing call*/ ) Native.check(st, logger) // checkLt / check fire here
    }
    call(0, null, null, null)
    if (result(0) != 1) return None
    val count = result(2).toInt
    val os = new Array[Int](count); val sr = new Array[Int](count); val sv = new Array[Int](count)
    if (count > 0) call(count, os, sr, sv)
    Some(Recovered(os, sv, result(4).toInt))
  }
}

// multipaxos.Leader's Phase 1: feed it every Phase1b; Some(phase2as, nextSlot) is what the handler sends and sets
class GpuLeaderRecovery(logger: Logger, handle: Long, round: Int, chosenWatermark: Int, gridCols: Int = 0, flags: Int = 0) {
  private val core = new GpuLeaderRecoveryCore(logger, handle, round, chosenWatermark, 0, -1, gridCols, flags)
  private val values = mutable.ArrayBuffer[CommandBatchOrNoop]()
  private def intern(v: CommandBatchOrNoop): Int = if (v.value.isNoop) -1 else { values += v; values.size - 1 }

  def handlePhase1b(p: Phase1b): Option[(Seq[Phase2a], Int)] = {
    core.append(p.round, p.groupIndex, p.acceptorIndex, p.info.map(i => (i.slot, i.voteRound, intern(i.voteValue))))
    core.tryRecover().map { r =>
      val phase2as = for (j <- r.slots.indices) yield Phase2a(
        slot = r.slots(j), round = round,
        commandBatchOrNoop = if (r.valueIds(j) < 0) CommandBatchOrNoop().withNoop(Noop()) else values(r.valueIds(j)))
      (phase2as, r.nextSlot)                                                          // Leader.scala:553-569
    }
  }
}

// ---- the replica's log and read path: a helper, not an actor (like GpuLeaderRecovery).  It buffers a tick's decoded
// ReplicaInbounds, puts the reads that are still deferred in front of them, hands the burst to fpx_replica_inbox and
// returns the schedule multipaxos.Replica would have followed message by message (Replica.scala:394-413, 455-529,
// 572-590, 629-690): for every slot executed this tick its value, then the reads released there, and the reads that ran
// at once in between.  The state machine, the client table, the routing of ClientReply / ReadReply and the recover timer
// stay with the caller, and so does sending the ChosenWatermarks this helper says are due.  `handle` is a MultiPaxos
// context (one leader group) that holds this replica's log.
class GpuReplicaLog(logger: Logger, handle: Long, index: Int, numReplicas: Int, sendChosenWatermarkEveryNEntries: Int) {
  // one read request as it arrived: a single command or a whole batch (one message, one slot, one fate)
  case class Read(kind: Int, slot: Int, src: Any, commands: Seq[Command])
  // a step of the schedule, in the order the reference takes them
  sealed trait Step
  case class Execute(slot: Int, value: CommandBatchOrNoop) extends Step
  // replySlot: what executeRead puts into ReadReply.slot (executedWatermark - 1 as it stands when the read runs: r - 1
  // for a read released under slot r, because executeLog has not incremented the watermark yet, :405-413, 526)
  case class RunRead(read: Read, replySlot: Int) extends Step
  case class Tick(steps: Seq[Step], chosenWatermarks: Seq[Int], executedWatermark: Int, numChosen: Int)

  private val kinds = mutable.ArrayBuffer[Int](); private val slots = mutable.ArrayBuffer[Int]()
  private val chosen = mutable.ArrayBuffer[CommandBatchOrNoop]()        // value id = position here
  private val valueIds = mutable.ArrayBuffer[Int]()
  private val reads = mutable.ArrayBuffer[Read]()                       // by message index (null for a Chosen)
  private var deferred = Vector[Read]()                                 // still deferred, in hand-back order
  // the values in the log above the watermark (the device holds their ids only for the burst that put them)
  private val held = mutable.Map[Int, CommandBatchOrNoop]()

  private def add(kind: Int, slot: Int, valueId: Int, read: Read): Unit = {
    kinds += kind; slots += slot; valueIds += valueId; reads += read
  }

  def receive(src: Any, inbound: ReplicaInbound): Unit = {
    import ReplicaInbound.Request
    inbound.request match {
      case Request.Chosen(c) =>
        chosen += c.commandBatchOrNoop
        add(4 /*FPX_WIRE_CHOSEN*/, c.slot, chosen.size - 1, null)
      case Request.ReadRequest(r)                => add(12, r.slot, -1, Read(12, r.slot, src, Seq(r.command)))
      case Request.SequentialReadRequest(r)      => add(13, r.slot, -1, Read(13, r.slot, src, Seq(r.command)))
      case Request.EventualReadRequest(r)        => add(14, -1, -1, Read(14, -1, src, Seq(r.command)))
      case Request.ReadRequestBatch(r)           => add(24, r.slot, -1, Read(24, r.slot, src, r.command))
      case Request.SequentialReadRequestBatch(r) => add(25, r.slot, -1, Read(25, r.slot, src, r.command))
      case Request.EventualReadRequestBatch(r)   => add(26, -1, -1, Read(26, -1, src, r.command))
      case Request.Empty                         => logger.fatal("Empty ReplicaInbound encountered.")
    }
  }

  // the tick: everything received since the last one, behind the reads still deferred
  def flush(): Tick = {
    val burstReads = deferred ++ reads
    val k = deferred.map(_.kind).toArray ++ kinds; val s = deferred.map(_.slot).toArray ++ slots
    val v = Array.fill(deferred.size)(-1) ++ valueIds
    val n = k.length
    val (exec, reply, order) = (new Array[Int](n), new Array[Int](n), new Array[Int](n))
    val (counts, state) = (new Array[Int](4), new Array[Int](2))
    Native.check(Native.replicaInbox(handle, n, k, s, v, null, exec, reply, order, counts, state), logger)
    val (numReads, ran, w0, w1) = (counts(0), counts(1), counts(2), counts(3))
    // the value of every slot executed this tick: put by this burst, or in the log from an earlier one
    val put = mutable.Map[Int, CommandBatchOrNoop]()
    // (a Chosen below W0 is a duplicate of an executed slot; the first Chosen of a slot is the one that was put)
    for (i <- 0 until n if k(i) == 4 && s(i) >= w0 && !put.contains(s(i)) && !held.contains(s(i))) put(s(i)) = chosen(v(i))
    held ++= put
    val steps = mutable.ArrayBuffer[Step]()
    var next = 0                                                        // into order(0 until ran)
    def runReadsUpTo(executed: Int): Unit =
      while (next < ran && exec(order(next)) <= executed) {
        steps += RunRead(burstReads(order(next)), reply(order(next))); next += 1
      }
    runReadsUpTo(w0)
    val watermarks = mutable.ArrayBuffer[Int]()
    for (slot <- w0 until w1) {
      steps += Execute(slot, held.remove(slot).get)
      runReadsUpTo(slot + 1)
      // Replica.scala:425-427, after executedWatermark += 1
      val wm = slot + 1
      if (wm % sendChosenWatermarkEveryNEntries == 0 && (wm / sendChosenWatermarkEveryNEntries) % numReplicas == index)
        watermarks += wm
    }
    deferred = (ran until numReads).map(j => burstReads(order(j))).toVector
    kinds.clear(); slots.clear(); valueIds.clear(); reads.clear(); chosen.clear()
    Tick(steps.toSeq, watermarks.toSeq, state(0), state(1))
  }
}

// Stands where a ProxyLeader stands (ProxyLeaderMain): Leaders keep sending Phase2a to it exactly as they send
// to a ProxyLeader (multipaxos/Leader.scala:364-398); replicas keep receiving Chosen from it.
class GpuProxyLeader[Transport <: frankenpaxos.Transport[Transport]](
    address: Transport#Address,
    transport: Transport,
    logger: Logger,
    config: Config[Transport],
    engine: GpuPhase2Engine[Transport],
    // true: the acceptors are the reference's own Acceptor actors somewhere else.  A Phase2a is opened on the device and
    // forwarded to f + 1 acceptors of its slot's group (or a grid column), their Phase2bs are buffered and tallied on
    // the device once per tick.  false: every acceptor lives in `engine` (the fused step) and no Phase2b ever arrives
    remoteAcceptors: Boolean = false
) extends Actor(address, transport, logger) {
  override type InboundMessage = ProxyLeaderInbound
  override val serializer = ProxyLeaderInboundSerializer

  private val roundSystem = new RoundSystem.ClassicRoundRobin(config.numLeaders)
  private val leaders = for (a <- config.leaderAddresses) yield chan[Leader[Transport]](a, Leader.serializer)
  private val replicas = for (a <- config.replicaAddresses) yield chan[Replica[Transport]](a, Replica.serializer)
  private val pending = mutable.Buffer[Phase2a]()
  private val pendingPhase2bs = mutable.Buffer[Phase2b]()
  private val acceptors =
    for (group <- config.acceptorAddresses) yield for (a <- group) yield chan[Acceptor[Transport]](a, Acceptor.serializer)

  // one tick: a zero-delay timer, i.e. "after the messages already queued on the event loop"
  private val tick = timer("gpuPhase2Tick", java.time.Duration.ZERO, () => flushTick())

  override def receive(src: Transport#Address, inbound: ProxyLeaderInbound): Unit = {
    inbound.request match {
      case ProxyLeaderInbound.Request.Phase2A(p) =>
        if (pending.isEmpty && pendingPhase2bs.isEmpty) tick.start()
        pending += p
      case ProxyLeaderInbound.Request.Phase2B(b) =>
        if (!remoteAcceptors)
          logger.fatal("GpuProxyLeader tallies on the device; it never receives Phase2b messages.")
        if (pending.isEmpty && pendingPhase2bs.isEmpty) tick.start()
        pendingPhase2bs += b
      case ProxyLeaderInbound.Request.Empty =>
        logger.fatal("Empty ProxyLeaderInbound encountered.")
    }
  }

  private def flushTick(): Unit = {
    if (remoteAcceptors) {
      flushRemoteTick()
      return
    }
    val result = engine.phase2Tick(pending.toList)
    pending.clear()
    for (c <- result.chosen) replicas.foreach(_.send(ReplicaInbound().withChosen(c)))
    for ((round, nack) <- result.nacks)
      leaders(roundSystem.leader(round)).send(LeaderInbound().withNack(nack))
  }

  // the tick among remote acceptors: the Phase2as first (a Phase2b of this tick may answer a Phase2a of this tick only
  // if an acceptor was faster than the event loop; opening first keeps it known either way), then the Phase2bs
  private def flushRemoteTick(): Unit = {
    val fresh = engine.openPhase2as(pending.toList)
    pending.clear()
    for (p <- fresh) {
      // ProxyLeader.scala:186-211: f + 1 acceptors of the slot's group, or a random write quorum of the grid (a column)
      val quorum =
        if (!config.flexible) scala.util.Random.shuffle(acceptors(p.slot % config.numAcceptorGroups)).take(config.f + 1)
        else {
          val col = scala.util.Random.nextInt(engine.perGroup)
          acceptors.map(_(col))
        }
      quorum.foreach(_.send(AcceptorInbound().withPhase2A(p)))
    }
    val chosen = engine.tallyPhase2bs(pendingPhase2bs.toList)
    pendingPhase2bs.clear()
    for (c <- chosen) replicas.foreach(_.send(ReplicaInbound().withChosen(c)))          // ProxyLeader.scala:246-253
  }
}

// Stands at ONE acceptor address (AcceptorMain); every acceptor address of the deployment gets one, all over the
// same engine.  The Leader's Phase1a goes to acceptor addresses (multipaxos/Leader.scala:410-420): without an
// actor here a new leader would never finish Phase 1.
class GpuAcceptor[Transport <: frankenpaxos.Transport[Transport]](
    address: Transport#Address,
    transport: Transport,
    logger: Logger,
    config: Config[Transport],
    engine: GpuPhase2Engine[Transport]
) extends Actor(address, transport, logger) {
  override type InboundMessage = AcceptorInbound
  override val serializer = AcceptorInboundSerializer

  logger.check(config.acceptorAddresses.flatten.contains(address))
  private val groupIndex = config.acceptorAddresses.indexWhere(_.contains(address))
  private val index = config.acceptorAddresses(groupIndex).indexOf(address)
  private val roundSystem = new RoundSystem.ClassicRoundRobin(config.numLeaders)
  // one tick, as GpuProxyLeader's: "after the messages already queued on the event loop" -- the burst that the proxy
  // leaders, leaders, clients and read batchers sent to the acceptor addresses of this engine
  private val inboxTick = timer("gpuAcceptorInboxTick", java.time.Duration.ZERO, () => engine.flushInbox())

  override def receive(src: Transport#Address, inbound: AcceptorInbound): Unit = {
    // enqueued, not answered: one tick flushes the burst through ONE native call (engine.flushInbox)
    val reply: engine.InboxReply => Unit = inbound.request match {
      case AcceptorInbound.Request.Phase1A(_) =>
        val leader = chan[Leader[Transport]](src, Leader.serializer)
        ({
          case engine.Nacked(nack)      => leader.send(LeaderInbound().withNack(nack))        // Acceptor.scala:155-162
          case engine.Promised(phase1b) => leader.send(LeaderInbound().withPhase1B(phase1b))  // Acceptor.scala:163-181
          case other                    => logger.fatal(s"Phase1a answered with $other")
        })
      case AcceptorInbound.Request.Phase2A(phase2a) =>
        ({
          case engine.Nacked(nack) =>                                                         // Acceptor.scala:192-199
            chan[Leader[Transport]](config.leaderAddresses(roundSystem.leader(phase2a.round)), Leader.serializer)
              .send(LeaderInbound().withNack(nack))
          case engine.Voted(phase2b) =>                                                       // Acceptor.scala:211-219
            chan[ProxyLeader[Transport]](src, ProxyLeader.serializer).send(ProxyLeaderInbound().withPhase2B(phase2b))
          case other => logger.fatal(s"Phase2a answered with $other")
        })
      case AcceptorInbound.Request.MaxSlotRequest(r) =>                                       // Acceptor.scala:222-237
        ({
          case engine.MaxVotedSlot(slot) =>
            chan[Client[Transport]](src, Client.serializer).send(
              ClientInbound().withMaxSlotReply(
                MaxSlotReply(commandId = r.commandId, groupIndex = groupIndex, acceptorIndex = index, slot = slot)))
          case other => logger.fatal(s"MaxSlotRequest answered with $other")
        })
      case AcceptorInbound.Request.BatchMaxSlotRequest(r) =>                                  // Acceptor.scala:239-254
        ({
          case engine.MaxVotedSlot(slot) =>
            chan[ReadBatcher[Transport]](src, ReadBatcher.serializer).send(
              ReadBatcherInbound().withBatchMaxSlotReply(
                BatchMaxSlotReply(readBatcherIndex = r.readBatcherIndex, readBatcherId = r.readBatcherId,
                                  acceptorIndex = index, slot = slot)))
          case other => logger.fatal(s"BatchMaxSlotRequest answered with $other")
        })
      case AcceptorInbound.Request.Empty =>
        logger.fatal("Empty AcceptorInbound encountered.")
    }
    if (engine.enqueueInbox(groupIndex, index, inbound.request, reply)) inboxTick.start()
  }
}
