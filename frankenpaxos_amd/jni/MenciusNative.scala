// MenciusNative.scala -- the Mencius half of the reference-side binding (source only, like Native.scala: no JDK /
// scalac in this image).  Drop into jvm/src/main/scala/frankenpaxos/gpu/ next to Native.scala.
//
//   GpuMenciusEngine       ONE libfpx context = the acceptors of every acceptor group of every leader group + the proxy
//                          leader's tallies, for a deployment whose acceptors and proxy leaders run in one process on
//                          the GPU box (one Transport event loop: not thread-safe, like every actor).  Log window, value
//                          garbage collection and thrifty target windows as in GpuPhase2Engine (Native.scala).
//   GpuMenciusProxyLeader  stands where a mencius.ProxyLeader stands (mencius/ProxyLeaderMain.scala): leaders of EVERY
//                          leader group keep sending it Phase2a and Phase2aNoopRange (mencius/Leader.scala:342-345, 455).
//                          remoteAcceptors = true: the acceptors are the reference's own, elsewhere -- the proxy leader
//                          forwards to them, and tallies their Phase2b / Phase2bNoopRange messages a tick at a time on the
//                          device (fpx_mencius_phase2b_tick; mencius/ProxyLeader.scala:216-411)
//   GpuMenciusAcceptor     stands at ONE acceptor address (mencius/AcceptorMain.scala); every acceptor address gets one,
//                          all over the same engine.  A Mencius Leader sends Phase1a to ACCEPTOR addresses
//                          (mencius/Leader.scala:486-491, resend timer :288-297): without an actor there a new leader
//                          would never finish Phase 1 (mencius/Acceptor.scala:166-200).  hostsPhase2 = true: the
//                          acceptor stands among the REFERENCE's mencius.ProxyLeaders and answers their per-acceptor
//                          Phase2a / Phase2aNoopRange too, a tick's burst in one device call
//                          (fpx_mencius_acceptor_inbox; mencius/Acceptor.scala:142-291)
//
// The walk of both on wire bytes -- a leader change in one leader group beside an undisturbed one, commands and noop
// ranges, Nacks to LeaderInbound field 7 -- is tests/test_jni_shim.py::test_a_mencius_leader_change_on_wire_bytes_...
// (mock JVM, against the oracle).
//
// The context's rows are leader-group-major in HBM (include/fpx.h, FPX_F_SLOT_MAJOR_ROWS): a run of commands is handed
// over AS THE LEADER GROUPS' BATCHES BACK TO BACK, each in slot order (a bucket per leader group, which is also the order
// in which one leader's messages arrive).
package frankenpaxos.gpu

import frankenpaxos.Actor
import frankenpaxos.Chan
import frankenpaxos.Logger
import frankenpaxos.mencius._
import frankenpaxos.roundsystem.RoundSystem
import scala.collection.mutable

class GpuMenciusEngine[Transport <: frankenpaxos.Transport[Transport]](
    logger: Logger,
    config: Config[Transport],
    numSlots: Int = 1 << 22,
    retainSlots: Int = 1 << 20,
    thrifty: Boolean = true               // mencius/ProxyLeader.scala:236: rand.shuffle(group).take(config.quorumSize)
) {
  config.checkValid()
  val L: Int = config.numLeaderGroups
  val A: Int = config.acceptorAddresses(0).size            // acceptor groups per leader group
  val R: Int = config.acceptorAddresses(0)(0).size         // acceptors per group (2f + 1)
  // a row keeps its leader group and its acceptor group when the log wraps: slot % L and (slot / L) % A are those of
  // slot % numSlots
  logger.check(numSlots % (L * A) == 0)
  private val chunk = math.max(L * A, numSlots / 16 / (L * A) * (L * A))
  logger.check(retainSlots + 2 * chunk <= numSlots)
  // fpx_config as fpx_jni.c reads it: slots, replicas, groups, leader groups, f, quorum kind, grid rows / cols,
  // leaders per group, ballot model (ACCEPTOR: noop ranges act on the acceptor's round), tally ways, replica base /
  // total, device, flags
  private val handle = Native.create(
    Array(numSlots, R, A, L, config.f, /*THRESHOLD*/ 0, 0, 0, config.leaderAddresses(0).size, /*ACCEPTOR*/ 0, 4, 0, 0, 0, 0))
  if (handle < 0) Native.check((-handle).toInt, logger)

  def leaderGroupOf(slot: Int): Int = slot % L                       // mencius/ProxyLeader.scala:169-176
  def ctxGroup(leaderGroup: Int, acceptorGroup: Int): Int = leaderGroup * A + acceptorGroup

  // ---- value ids, the window: as GpuPhase2Engine (an id lives as long as the row it was proposed in)
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

  private var base = 0
  private val chosenInWindow = new java.util.BitSet(numSlots)
  private var chosenPrefix = 0
  private var highestChosen = -1
  private def row(slot: Int): Int = slot % numSlots
  private def slotOfRow(r: Int): Int = base + ((r - row(base)) % numSlots + numSlots) % numSlots
  private def markChosen(slot: Int): Unit = {
    chosenInWindow.set(row(slot))
    highestChosen = math.max(highestChosen, slot)
    while (chosenPrefix < base + numSlots && chosenInWindow.get(row(chosenPrefix))) chosenPrefix += 1
  }
  private def advanceWindow(): Boolean = {
    var moved = false
    while (chosenPrefix - base >= chunk && highestChosen - (base + chunk) >= retainSlots) {
      val r0 = row(base)
      Native.check(Native.recycleSlots(handle, r0, chunk), logger)   // votes dropped, tallies (ranges too) forgotten
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
  def inWindow(slot: Int): Boolean = slot >= base && slot < base + numSlots

  // ---- thrifty targets: a window of quorumSize neighbouring acceptors of the slot's group, rotating (any quorumSize of
  // them will do, mencius/ProxyLeader.scala:236)
  private var rotor = 0
  private def thriftyMask(masks: Array[Long], at: Int): Unit = {
    val start = rotor % R
    rotor += 1
    for (j <- 0 until config.quorumSize) { val a = (start + j) % R; masks(at + (a >> 6)) |= 1L << (a & 63) }
  }

  case class Result(chosen: Seq[Chosen], chosenRanges: Seq[ChosenNoopRange], nacks: Seq[(Int, Int, Nack)]) // (slot, round, Nack)

  // ---- one run of commands: mencius.ProxyLeader.handlePhase2a + every mencius.Acceptor.handlePhase2a +
  // mencius.ProxyLeader.handlePhase2b (mencius/ProxyLeader.scala:216-253, 305-353, mencius/Acceptor.scala:202-235)
  private val deferred = mutable.Queue[Phase2a]()
  def commands(incoming: Seq[Phase2a]): Result = {
    val chosenOut = mutable.Buffer[Chosen](); val nackOut = mutable.Buffer[(Int, Int, Nack)]()
    var batch: Seq[Phase2a] = deferred.dequeueAll(_ => true) ++ incoming
    while (batch.nonEmpty) {
      val (nowAny, later) = batch.filter(_.slot >= base).partition(_.slot < base + numSlots)
      // the leader groups' batches back to back, each in slot order; one leader's own messages keep their order
      // (sortBy is stable), messages of different leader groups were in flight together anyway
      val now = nowAny.groupBy(p => leaderGroupOf(p.slot)).toSeq.sortBy(_._1).flatMap(_._2.sortBy(_.slot)).toArray
      val n = now.length
      if (n > 0) {
        val slot = now.map(p => row(p.slot)); val round = now.map(_.round)
        val value = now.map(p => intern(row(p.slot), p.commandBatchOrNoop))
        val masks: Array[Long] = if (thrifty && R > config.quorumSize) {
          val m = new Array[Long](4 * n); for (i <- 0 until n) thriftyMask(m, 4 * i); m
        } else null
        val chosen = new Array[Byte](n); val cr = new Array[Int](n); val cv = new Array[Int](n); val nr = new Array[Int](n)
        Native.check(Native.phase2Fused(handle, n, slot, round, value, masks, chosen, cr, cv, nr), logger)
        for (i <- 0 until n) {
          if (chosen(i) != 0) {                              // mencius/ProxyLeader.scala:338-352
            chosenOut += Chosen(slot = now(i).slot, commandBatchOrNoop = valueOf(cv(i)))
            markChosen(now(i).slot)
          }
          if (nr(i) >= 0) nackOut += ((now(i).slot, round(i), Nack(round = nr(i))))   // mencius/Acceptor.scala:208-219
        }
      }
      batch = if (advanceWindow()) later else { deferred ++= later; Seq.empty }
    }
    Result(chosenOut, Seq.empty, nackOut)
  }

  // ---- one run of noop ranges: the *NoopRange handlers (mencius/ProxyLeader.scala:255-303, 355-411,
  // mencius/Acceptor.scala:237-291), one fused launch (up to 4096 of them walk the chain in one workgroup).  A range is
  // cut at the end of the window; what lies beyond waits like a command beyond the window does
  private val deferredRanges = mutable.Queue[Phase2aNoopRange]()
  def ranges(incoming: Seq[Phase2aNoopRange]): Result = {
    val chosenOut = mutable.Buffer[ChosenNoopRange](); val nackOut = mutable.Buffer[(Int, Int, Nack)]()
    var batch: Seq[Phase2aNoopRange] = deferredRanges.dequeueAll(_ => true) ++ incoming
    while (batch.nonEmpty) {
      val end = base + numSlots
      val now = mutable.Buffer[Phase2aNoopRange](); val later = mutable.Buffer[Phase2aNoopRange]()
      for (p <- batch if p.slotEndExclusive > base) {
        val lo = math.max(p.slotStartInclusive, base)          // (below the window: chosen long ago and recycled)
        if (lo >= end) later += p
        else if (p.slotEndExclusive <= end) now += p.copy(slotStartInclusive = lo)
        else { now += p.copy(slotStartInclusive = lo, slotEndExclusive = end); later += p.copy(slotStartInclusive = end) }
      }
      val m = now.size
      if (m > 0) {
        // rows: a range inside the window is one run of rows of its leader group unless the window wraps inside it --
        // then it is handed over as two ranges
        val parts = now.flatMap { p =>
          val (a, b) = (row(p.slotStartInclusive), row(p.slotEndExclusive - 1) + 1)
          if (a < b) Seq((p, a, b)) else Seq((p, a, numSlots), (p, leaderGroupOf(p.slotStartInclusive), b)).filter(x => x._2 < x._3)
        }
        val k = parts.size
        val start = parts.map(_._2).toArray; val stop = parts.map(_._3).toArray; val round = parts.map(_._1.round).toArray
        val isNew = new Array[Byte](k); val chosen = new Array[Byte](k); val nr = new Array[Int](k)
        val votes = new Array[Long](k * A * 4); val nacks = new Array[Long](k * A * 4)
        Native.check(Native.noopRangesFused(handle, k, A, start, stop, round, null, votes, nacks, nr, isNew, chosen), logger)
        for (((p, _, _), i) <- parts.zipWithIndex) {
          if (chosen(i) != 0) {                              // mencius/ProxyLeader.scala:395-407
            chosenOut += ChosenNoopRange(slotStartInclusive = slotOfRow(start(i)), slotEndExclusive = slotOfRow(start(i)) + (stop(i) - start(i)))
            var s = slotOfRow(start(i))
            while (s < slotOfRow(start(i)) + (stop(i) - start(i))) { if (leaderGroupOf(s) == leaderGroupOf(p.slotStartInclusive)) markChosen(s); s += 1 }
          }
          if (nr(i) >= 0) nackOut += ((p.slotStartInclusive, round(i), Nack(round = nr(i))))   // mencius/Acceptor.scala:245-256
        }
      }
      batch = if (advanceWindow()) later else { deferredRanges ++= later; Seq.empty }
    }
    Result(Seq.empty, chosenOut, nackOut)
  }

  // ---- a proxy leader among REMOTE acceptors (GpuMenciusProxyLeader, remoteAcceptors = true): only the proxy leader's
  // tallies live in the context.  The window must cover the slots in flight: a key that lies outside it, or a range that
  // wraps around it, is fatal here (the colocated path defers and cuts; a remote acceptor answers with the key it was
  // sent, so the key cannot be cut).
  private def remoteRow(slot: Int): Int = {
    if (!inWindow(slot)) { advanceWindow(); if (!inWindow(slot)) logger.fatal(s"slot $slot lies outside the window at $base") }
    row(slot)
  }
  private def remoteRangeRows(start: Int, end: Int): (Int, Int) = {
    if (end > start) { remoteRow(start); remoteRow(end - 1) }
    val a = row(start)
    if (a + (end - start) > numSlots) logger.fatal(s"range [$start, $end) wraps around the window")
    (a, a + (end - start))
  }

  // mencius/ProxyLeader.scala:216-253 without the relay: the Phase2as that are new (to be forwarded), in order
  def openCommands(incoming: Seq[Phase2a]): Seq[Phase2a] = {
    val n = incoming.size
    if (n == 0) return Seq.empty
    val slot = incoming.map(p => remoteRow(p.slot)).toArray; val round = incoming.map(_.round).toArray
    val value = incoming.map(p => intern(row(p.slot), p.commandBatchOrNoop)).toArray
    val isNew = new Array[Byte](n)
    Native.check(Native.proxyOpen(handle, n, slot, round, value, isNew), logger)
    incoming.indices.filter(isNew(_) != 0).map(incoming)
  }

  // mencius/ProxyLeader.scala:255-303 without the relay
  def openRanges(incoming: Seq[Phase2aNoopRange]): Seq[Phase2aNoopRange] = {
    val n = incoming.size
    if (n == 0) return Seq.empty
    val rows = incoming.map(p => remoteRangeRows(p.slotStartInclusive, p.slotEndExclusive))
    val isNew = new Array[Byte](n)
    Native.check(Native.proxyOpenNoopRanges(handle, n, rows.map(_._1).toArray, rows.map(_._2).toArray,
                                            incoming.map(_.round).toArray, isNew), logger)
    incoming.indices.filter(isNew(_) != 0).map(incoming)
  }

  // mencius/ProxyLeader.scala:305-411 for one tick of Phase2b (Left) and Phase2bNoopRange (Right) messages in arrival
  // order: ONE native call; the Chosen / ChosenNoopRange to send, in message order
  def tallyPhase2bs(msgs: Seq[Either[Phase2b, Phase2bNoopRange]]): Seq[Either[Chosen, ChosenNoopRange]] = {
    val n = msgs.size
    if (n == 0) return Seq.empty
    val kind = new Array[Int](n); val group = new Array[Int](n); val acceptor = new Array[Int](n)
    val slot = new Array[Int](n); val slotEnd = new Array[Int](n); val round = new Array[Int](n)
    for ((m, i) <- msgs.zipWithIndex) m match {
      case Left(p) =>
        kind(i) = Native.WIRE_PHASE2B; acceptor(i) = p.acceptorIndex; slot(i) = remoteRow(p.slot); slotEnd(i) = -1
        round(i) = p.round
      case Right(p) =>
        val (a, b) = remoteRangeRows(p.slotStartInclusive, p.slotEndExclusive)
        kind(i) = Native.WIRE_PHASE2B_NOOP_RANGE; group(i) = p.acceptorGroupIndex; acceptor(i) = p.acceptorIndex
        slot(i) = a; slotEnd(i) = b; round(i) = p.round
    }
    // at most one record per message
    val oKind = new Array[Int](n); val oSlot = new Array[Int](n); val oEnd = new Array[Int](n)
    val oRound = new Array[Int](n); val oValue = new Array[Int](n); val count = new Array[Int](1)
    Native.check(Native.menciusPhase2bTick(handle, n, kind, group, acceptor, slot, slotEnd, round, oKind, oSlot, oEnd, oRound,
                                           oValue, n, count), logger)
    for (k <- 0 until count(0)) yield {
      val s = slotOfRow(oSlot(k))
      if (oKind(k) == Native.WIRE_PHASE2B) {                  // mencius/ProxyLeader.scala:335-351
        markChosen(s)
        Left(Chosen(slot = s, commandBatchOrNoop = valueOf(oValue(k))))
      } else {                                               // :395-407
        val e = s + (oEnd(k) - oSlot(k))
        var t = s
        while (t < e) { markChosen(t); t += L }               // the leader group's own slots
        Right(ChosenNoopRange(slotStartInclusive = s, slotEndExclusive = e))
      }
    }
  }

  // ---- Phase 1, acceptor side (mencius/Acceptor.scala:166-200)
  def handlePhase1a(leaderGroup: Int, acceptorGroup: Int, index: Int, phase1a: Phase1a): Either[Nack, Phase1b] = {
    val g = ctxGroup(leaderGroup, acceptorGroup)
    val target = new Array[Long](4); target(index >> 6) = 1L << (index & 63)
    val bits = new Array[Long](8)
    // rows, not slots (see GpuPhase2Engine.handlePhase1a): promise from row 0 on, filter the info by slot below
    Native.check(Native.acceptorPhase1a(handle, g, phase1a.round, 0, target, bits), logger)
    if ((bits(4 + (index >> 6)) & (1L << (index & 63))) != 0)
      return Left(Nack(round = Native.acceptorRound(handle, g, index)))               // :173-180
    var cap = 1024
    var slots = new Array[Int](cap); var vr = new Array[Int](cap); var vv = new Array[Int](cap)
    var k = Native.acceptorPhase1bInfo(handle, g, index, 0, cap, slots, vr, vv)
    if (k > cap) {
      cap = k; slots = new Array[Int](cap); vr = new Array[Int](cap); vv = new Array[Int](cap)
      k = Native.acceptorPhase1bInfo(handle, g, index, 0, cap, slots, vr, vv)
    }
    if (k < 0) Native.check(-k, logger)
    val info = (0 until k)                                                             // :184-199
      .map(j => Phase1bSlotInfo(slot = slotOfRow(slots(j)), voteRound = vr(j), voteValue = valueOf(vv(j))))
      .filter(_.slot >= phase1a.chosenWatermark)
      .sortBy(_.slot)
    Right(Phase1b(groupIndex = acceptorGroup, acceptorIndex = index, round = phase1a.round, info = info))
  }

  // ---- Phase 1 for a burst of Phase1as, as GpuPhase2Engine's: a new leader of a leader group sends one to every
  // acceptor address of that group (mencius/Leader.scala:486-491), and they arrive together.  The GpuMenciusAcceptors
  // enqueue them here; the zero-delay timer of the first one flushes the burst: maximal runs of equal
  // (round, chosenWatermark), ONE native call per run (fpx_acceptor_phase1 over the L * A context groups, only the
  // addressed ones with a non-empty mask), each acceptor answered from its slice.  As in handlePhase1a the call runs with
  // watermark row 0; the per-slot filter and slotOfRow stay here.
  private val pendingPhase1as = mutable.Buffer[(Int, Int, Int, Phase1a, Either[Nack, Phase1b] => Unit)]()

  // true: the queue was empty -- the caller starts its tick
  def enqueuePhase1a(leaderGroup: Int, acceptorGroup: Int, index: Int, phase1a: Phase1a,
                     reply: Either[Nack, Phase1b] => Unit): Boolean = {
    val first = pendingPhase1as.isEmpty
    pendingPhase1as += ((leaderGroup, acceptorGroup, index, phase1a, reply))
    first
  }

  def flushPhase1as(): Unit = {
    var rest = pendingPhase1as.toList
    pendingPhase1as.clear()
    while (rest.nonEmpty) {
      val key = (rest.head._4.round, rest.head._4.chosenWatermark)
      val (run, later) = rest.span(m => (m._4.round, m._4.chosenWatermark) == key)
      rest = later
      if (run.size == 1) run.head._5(handlePhase1a(run.head._1, run.head._2, run.head._3, run.head._4))   // a lone message
      else phase1Run(run)
    }
  }

  private def phase1Run(run: List[(Int, Int, Int, Phase1a, Either[Nack, Phase1b] => Unit)]): Unit = {
    val phase1a = run.head._4
    val ctxGroups = L * A
    val words = 4 * ctxGroups
    val target = new Array[Long](words)
    for ((l, a, i, _, _) <- run) target(4 * ctxGroup(l, a) + (i >> 6)) |= 1L << (i & 63)
    val bits = new Array[Long](2 * words)
    val offsets = new Array[Long](ctxGroups * R + 1)
    var cap = 1024 * run.size
    var slots = new Array[Int](cap); var vr = new Array[Int](cap); var vv = new Array[Int](cap)
    var k = Native.acceptorPhase1All(handle, phase1a.round, 0, ctxGroups, target, bits, cap, offsets, slots, vr, vv)
    if (k > cap) {
      // the promises hold; the same call again answers the same (a promiser promises its own round again)
      cap = k.toInt; slots = new Array[Int](cap); vr = new Array[Int](cap); vv = new Array[Int](cap)
      k = Native.acceptorPhase1All(handle, phase1a.round, 0, ctxGroups, target, bits, cap, offsets, slots, vr, vv)
    }
    if (k < 0) Native.check((-k).toInt, logger)
    for ((l, a, i, p, reply) <- run) {
      val g = ctxGroup(l, a)
      if ((bits(words + 4 * g + (i >> 6)) & (1L << (i & 63))) != 0) {
        reply(Left(Nack(round = Native.acceptorRound(handle, g, i))))                    // mencius/Acceptor.scala:173-180
      } else {
        val e = g * R + i
        val info = (offsets(e).toInt until offsets(e + 1).toInt)                         // :184-199
          .map(j => Phase1bSlotInfo(slot = slotOfRow(slots(j)), voteRound = vr(j), voteValue = valueOf(vv(j))))
          .filter(_.slot >= p.chosenWatermark)
          .sortBy(_.slot)
        reply(Right(Phase1b(groupIndex = a, acceptorIndex = i, round = p.round, info = info)))
      }
    }
  }

  // ---- the acceptors' inbox as a burst (fpx_mencius_acceptor_inbox), for acceptors hosted here among the REFERENCE's
  // mencius.ProxyLeaders.  Those send every Phase2a once per acceptor address to quorumSize acceptors of the slot's group,
  // and every Phase2aNoopRange once per acceptor address to quorumSize acceptors of every acceptor group of the leader
  // group (mencius/ProxyLeader.scala:216-303); now and then a leader's Phase1as lie between them.  The GpuMenciusAcceptors
  // (hostsPhase2 = true) enqueue whatever they receive here; the zero-delay timer of the first message flushes the queue:
  // ONE native call per burst, every acceptor answered from its message's reply, exactly as if each had handled its
  // messages one by one.  The call does not produce Phase1b.info -- a promise's info is the acceptor's votes as of that
  // message -- so a burst is cut after each maximal run of Phase1as, and the promisers of that run get their info from
  // acceptorPhase1All's slices (no vote lies between the promise and the end of the burst).  As for a proxy leader among
  // remote acceptors, the window must cover the slots in flight (remoteRow / remoteRangeRows).
  sealed trait InboxReply
  case class Voted(phase2b: Phase2b) extends InboxReply
  case class VotedRange(phase2b: Phase2bNoopRange) extends InboxReply
  case class Nacked(nack: Nack) extends InboxReply
  case class Promised(phase1b: Phase1b) extends InboxReply
  private case class InboxMsg(leaderGroup: Int, acceptorGroup: Int, index: Int, request: AcceptorInbound.Request,
                              reply: InboxReply => Unit) {
    def isPhase1a: Boolean = request.isPhase1A
  }
  private val pendingInbox = mutable.Buffer[InboxMsg]()

  // true: the queue was empty -- the caller starts its tick
  def enqueueInbox(leaderGroup: Int, acceptorGroup: Int, index: Int, request: AcceptorInbound.Request,
                   reply: InboxReply => Unit): Boolean = {
    val first = pendingInbox.isEmpty
    pendingInbox += InboxMsg(leaderGroup, acceptorGroup, index, request, reply)
    first
  }

  def flushInbox(): Unit = {
    var rest = pendingInbox.toList
    pendingInbox.clear()
    while (rest.nonEmpty) {
      val (head, tail) = rest.span(!_.isPhase1a)
      val (phase1as, later) = tail.span(_.isPhase1a)
      rest = later
      inboxBurst(head ++ phase1as, head.size)
    }
  }

  private def phase1bInfo(g: Int, index: Int, chosenWatermark: Int): Seq[Phase1bSlotInfo] = {
    var cap = 1024
    var slots = new Array[Int](cap); var vr = new Array[Int](cap); var vv = new Array[Int](cap)
    var k = Native.acceptorPhase1bInfo(handle, g, index, 0, cap, slots, vr, vv)
    if (k > cap) {
      cap = k; slots = new Array[Int](cap); vr = new Array[Int](cap); vv = new Array[Int](cap)
      k = Native.acceptorPhase1bInfo(handle, g, index, 0, cap, slots, vr, vv)
    }
    if (k < 0) Native.check(-k, logger)
    (0 until k)                                                                           // :184-199
      .map(j => Phase1bSlotInfo(slot = slotOfRow(slots(j)), voteRound = vr(j), voteValue = valueOf(vv(j))))
      .filter(_.slot >= chosenWatermark)
      .sortBy(_.slot)
  }

  // burst = any messages but Phase1as, then (from firstPhase1a on) a run of Phase1as
  private def inboxBurst(burst: List[InboxMsg], firstPhase1a: Int): Unit = {
    val n = burst.size
    val kind = new Array[Int](n); val group = new Array[Int](n); val acc = new Array[Int](n)
    val slot = Array.fill(n)(-1); val slotEnd = Array.fill(n)(-1); val round = Array.fill(n)(-1); val value = Array.fill(n)(-1)
    for ((m, i) <- burst.zipWithIndex) {
      group(i) = ctxGroup(m.leaderGroup, m.acceptorGroup); acc(i) = m.index
      m.request match {
        case AcceptorInbound.Request.Phase2A(p) =>
          kind(i) = Native.WIRE_PHASE2A; slot(i) = remoteRow(p.slot); round(i) = p.round
          value(i) = intern(row(p.slot), p.commandBatchOrNoop)
        case AcceptorInbound.Request.Phase2ANoopRange(p) =>
          val (a, b) = remoteRangeRows(p.slotStartInclusive, p.slotEndExclusive)
          kind(i) = Native.WIRE_PHASE2A_NOOP_RANGE; slot(i) = a; slotEnd(i) = b; round(i) = p.round
        case AcceptorInbound.Request.Phase1A(p) => kind(i) = Native.WIRE_PHASE1A; round(i) = p.round
        case AcceptorInbound.Request.Empty => logger.fatal("Empty AcceptorInbound encountered.")
      }
    }
    val replyKind = new Array[Int](n); val replyValue = new Array[Int](n)
    Native.check(Native.menciusAcceptorInbox(handle, n, kind, group, acc, slot, slotEnd, round, value, replyKind, replyValue),
                 logger)
    // everything but the promises, in delivery order
    for ((m, i) <- burst.zipWithIndex) {
      (m.request, replyKind(i)) match {
        case (_, Native.WIRE_NACK) => m.reply(Nacked(Nack(round = replyValue(i))))            // :173-180, :210-218, :245-256
        case (AcceptorInbound.Request.Phase2A(p), _) =>                                       // :220-234
          m.reply(Voted(Phase2b(acceptorIndex = m.index, slot = p.slot, round = p.round)))
        case (AcceptorInbound.Request.Phase2ANoopRange(p), _) =>                              // :279-290
          m.reply(VotedRange(Phase2bNoopRange(acceptorGroupIndex = m.acceptorGroup, acceptorIndex = m.index,
                                              slotStartInclusive = p.slotStartInclusive,
                                              slotEndExclusive = p.slotEndExclusive, round = p.round)))
        case _ => ()                                                                          // a promise: below
      }
    }
    // the promisers of the run of Phase1as, as GpuPhase2Engine.inboxBurst: the promises of an acceptor's last round per
    // (round, chosenWatermark) by acceptorPhase1All, an earlier promise of an acceptor that promised twice in one run by
    // acceptorPhase1bInfo -- the votes are the same
    val promisers = burst.zipWithIndex.drop(firstPhase1a).filter(mi => replyKind(mi._2) == Native.WIRE_PHASE1B).map(_._1)
    val lastRound = mutable.Map[(Int, Int, Int), Int]()
    for (m <- promisers) lastRound((m.leaderGroup, m.acceptorGroup, m.index)) = m.request.phase1A.get.round
    val (current, earlier) =
      promisers.partition(m => lastRound((m.leaderGroup, m.acceptorGroup, m.index)) == m.request.phase1A.get.round)
    for ((_, run) <- current.groupBy(_.request.phase1A.get.round).toSeq.sortBy(_._1))
      phase1Run(run.map(m => (m.leaderGroup, m.acceptorGroup, m.index, m.request.phase1A.get,
                              (r: Either[Nack, Phase1b]) => m.reply(r.fold(Nacked(_), Promised(_))))))
    for (m <- earlier) {
      val p = m.request.phase1A.get
      m.reply(Promised(Phase1b(groupIndex = m.acceptorGroup, acceptorIndex = m.index, round = p.round,
                               info = phase1bInfo(ctxGroup(m.leaderGroup, m.acceptorGroup), m.index, p.chosenWatermark))))
    }
  }

  def close(): Unit = Native.check(Native.destroy(handle), logger)
}

// mencius.Leader's Phase 1 among acceptors outside the leader's context (GpuLeaderRecoveryCore, Native.scala): the
// leader group's index and phase1.recoverSlot go in, and the slots that come out are the leader group's own
// (mencius/Leader.scala:582-659)
class GpuMenciusLeaderRecovery(logger: Logger, handle: Long, round: Int, chosenWatermark: Int, leaderGroup: Int,
                               recoverSlot: Int) {
  private val core = new GpuLeaderRecoveryCore(logger, handle, round, chosenWatermark, leaderGroup, recoverSlot, 0, 0)
  private val values = mutable.ArrayBuffer[CommandBatchOrNoop]()
  private def intern(v: CommandBatchOrNoop): Int = if (v.value.isNoop) -1 else { values += v; values.size - 1 }

  def handlePhase1b(p: Phase1b): Option[(Seq[Phase2a], Int)] = {
    core.append(p.round, p.groupIndex, p.acceptorIndex, p.info.map(i => (i.slot, i.voteRound, intern(i.voteValue))))
    core.tryRecover().map { r =>
      val phase2as = for (j <- r.slots.indices) yield Phase2a(
        slot = r.slots(j), round = round,
        commandBatchOrNoop = if (r.valueIds(j) < 0) CommandBatchOrNoop().withNoop(Noop()) else values(r.valueIds(j)))
      (phase2as, r.nextSlot)                                                          // Leader.scala:629-647
    }
  }
}

class GpuMenciusProxyLeader[Transport <: frankenpaxos.Transport[Transport]](
    address: Transport#Address,
    transport: Transport,
    logger: Logger,
    config: Config[Transport],
    engine: GpuMenciusEngine[Transport],
    // true: the acceptors are remote (the reference's mencius.Acceptor, or anything that speaks its protocol) -- this
    // actor relays Phase2a / Phase2aNoopRange to them and tallies their Phase2b / Phase2bNoopRange on the device
    remoteAcceptors: Boolean = false,
    seed: Long = System.identityHashCode(this)
) extends Actor(address, transport, logger) {
  override type InboundMessage = ProxyLeaderInbound
  override val serializer = ProxyLeaderInboundSerializer

  private val slotSystem = new RoundSystem.ClassicRoundRobin(config.numLeaderGroups)
  private val roundSystem = new RoundSystem.ClassicRoundRobin(config.leaderAddresses(0).size)
  private val leaders = for (group <- config.leaderAddresses)
    yield for (a <- group) yield chan[Leader[Transport]](a, Leader.serializer)
  private val replicas = for (a <- config.replicaAddresses) yield chan[Replica[Transport]](a, Replica.serializer)
  // config.acceptorAddresses(leaderGroup)(acceptorGroup)(index), mencius/ProxyLeader.scala:121-128
  private val acceptors =
    if (!remoteAcceptors) Seq.empty
    else for (groups <- config.acceptorAddresses) yield for (group <- groups)
      yield for (a <- group) yield chan[Acceptor[Transport]](a, Acceptor.serializer)
  private val rand = new scala.util.Random(seed)

  // the burst, in arrival order: Left = a command, Right = a noop range
  private val pending = mutable.Buffer[Either[Phase2a, Phase2aNoopRange]]()
  // remoteAcceptors: the acceptors' answers of the tick, in arrival order
  private val pendingPhase2bs = mutable.Buffer[Either[Phase2b, Phase2bNoopRange]]()
  private val tick = timer("gpuMenciusTick", java.time.Duration.ZERO, () => flushTick())
  private def enqueued(): Unit = if (pending.isEmpty && pendingPhase2bs.isEmpty) tick.start()

  override def receive(src: Transport#Address, inbound: ProxyLeaderInbound): Unit = {
    import ProxyLeaderInbound.Request
    inbound.request match {
      case Request.Phase2A(p) =>
        enqueued()
        pending += Left(p)
      case Request.Phase2ANoopRange(p) =>
        enqueued()
        pending += Right(p)
      case Request.HighWatermark(h) =>                       // mencius/ProxyLeader.scala:207-214
        for (group <- leaders; leader <- group) leader.send(LeaderInbound().withHighWatermark(h))
      case Request.Phase2B(p) if remoteAcceptors =>          // mencius/ProxyLeader.scala:305-353, tallied by the tick
        enqueued()
        pendingPhase2bs += Left(p)
      case Request.Phase2BNoopRange(p) if remoteAcceptors => // :355-411
        enqueued()
        pendingPhase2bs += Right(p)
      case Request.Phase2B(_) | Request.Phase2BNoopRange(_) =>
        logger.fatal("GpuMenciusProxyLeader tallies on the device; it never receives Phase2b messages.")
      case Request.Empty =>
        logger.fatal("Empty ProxyLeaderInbound encountered.")
    }
  }

  private def deliver(r: engine.Result): Unit = {
    for (c <- r.chosen) replicas.foreach(_.send(ReplicaInbound().withChosen(c)))
    for (c <- r.chosenRanges) replicas.foreach(_.send(ReplicaInbound().withChosenNoopRange(c)))
    for ((slot, round, nack) <- r.nacks)                     // mencius/Acceptor.scala:215-217
      leaders(slotSystem.leader(slot))(roundSystem.leader(round)).send(LeaderInbound().withNack(nack))
  }

  // The burst is cut into MAXIMAL RUNS of one kind, in arrival order: one native call per run.  A leader's own stream --
  // a command in round r, a noop range in round r' >= r, a command in r' -- reaches the acceptors in the order it was sent
  // (an earlier version flushed all commands, then all ranges: the range of a later round would have made the acceptors
  // Nack the same leader's earlier command).  Within a run of commands the leader groups' batches are regrouped (above).
  private def flushTick(): Unit = {
    var i = 0
    while (i < pending.size) {
      var j = i
      while (j < pending.size && pending(j).isLeft == pending(i).isLeft) j += 1
      val run = pending.slice(i, j)
      if (remoteAcceptors) relay(run)
      else deliver(if (pending(i).isLeft) engine.commands(run.map(_.left.get)) else engine.ranges(run.map(_.right.get)))
      i = j
    }
    pending.clear()
    if (pendingPhase2bs.nonEmpty) {
      // the tick's Phase2b and Phase2bNoopRange messages in ONE native call; Chosen / ChosenNoopRange to every replica in
      // record (= message) order (mencius/ProxyLeader.scala:335-351, 395-407)
      val out = engine.tallyPhase2bs(pendingPhase2bs)
      pendingPhase2bs.clear()
      for (c <- out) c match {
        case Left(chosen)  => replicas.foreach(_.send(ReplicaInbound().withChosen(chosen)))
        case Right(chosen) => replicas.foreach(_.send(ReplicaInbound().withChosenNoopRange(chosen)))
      }
    }
  }

  // remoteAcceptors: a run of one kind is opened on the device (a duplicate is not forwarded, :222-229, 262-271) and
  // relayed -- a command to quorumSize acceptors of its slot's acceptor group (:231-236), a range to quorumSize acceptors
  // of EVERY acceptor group of its leader group (:274-293)
  private def relay(run: Seq[Either[Phase2a, Phase2aNoopRange]]): Unit = {
    if (run.head.isLeft) {
      for (p <- engine.openCommands(run.map(_.left.get))) {
        val lg = slotSystem.leader(p.slot)
        val group = acceptors(lg)((p.slot / config.numLeaderGroups) % acceptors(lg).size)   // :169-176
        rand.shuffle(group).take(config.quorumSize).foreach(_.send(AcceptorInbound().withPhase2A(p)))
      }
    } else {
      for (p <- engine.openRanges(run.map(_.right.get)); group <- acceptors(slotSystem.leader(p.slotStartInclusive)))
        rand.shuffle(group).take(config.quorumSize).foreach(_.send(AcceptorInbound().withPhase2ANoopRange(p)))
    }
  }
}

class GpuMenciusAcceptor[Transport <: frankenpaxos.Transport[Transport]](
    address: Transport#Address,
    transport: Transport,
    logger: Logger,
    config: Config[Transport],
    engine: GpuMenciusEngine[Transport],
    // true: this acceptor stands among the REFERENCE's mencius.ProxyLeaders, which send Phase2a and Phase2aNoopRange to
    // acceptor addresses (mencius/ProxyLeader.scala:216-303): everything is enqueued and one tick flushes the burst
    // through ONE native call (engine.flushInbox).  false: only Phase1as arrive here (GpuMenciusProxyLeader holds the
    // acceptors), and a Phase2a / Phase2aNoopRange is fatal
    hostsPhase2: Boolean = false
) extends Actor(address, transport, logger) {
  override type InboundMessage = AcceptorInbound
  override val serializer = AcceptorInboundSerializer

  // config.acceptorAddresses(leaderGroup)(acceptorGroup)(index)
  private val (leaderGroup, acceptorGroup, index) = (for {
    (lg, l) <- config.acceptorAddresses.zipWithIndex
    (ag, a) <- lg.zipWithIndex
    (addr, i) <- ag.zipWithIndex
    if addr == address
  } yield (l, a, i)).head

  private val roundSystem = new RoundSystem.ClassicRoundRobin(config.leaderAddresses(leaderGroup).size)  // mencius/Acceptor.scala:104-106
  private val slotSystem = new RoundSystem.ClassicRoundRobin(config.numLeaderGroups)                      // :112-113
  private val leaders: Seq[Seq[Chan[Leader[Transport]]]] =
    for (group <- config.leaderAddresses) yield for (a <- group) yield chan[Leader[Transport]](a, Leader.serializer)

  // one tick, as GpuMenciusProxyLeader's: "after the messages already queued on the event loop" -- the Phase1as of a burst
  private val phase1Tick = timer("gpuMenciusPhase1Tick", java.time.Duration.ZERO, () => engine.flushPhase1as())
  // ... and with hostsPhase2 the whole burst the proxy leaders and leaders sent to the acceptor addresses of this engine
  private val inboxTick = timer("gpuMenciusInboxTick", java.time.Duration.ZERO, () => engine.flushInbox())

  override def receive(src: Transport#Address, inbound: AcceptorInbound): Unit = {
    if (hostsPhase2) receiveHosted(src, inbound) else receivePhase1Only(src, inbound)
  }

  // enqueued, not answered: one tick flushes the burst through ONE native call (engine.flushInbox)
  private def receiveHosted(src: Transport#Address, inbound: AcceptorInbound): Unit = {
    // a Nack goes to leaders(slotSystem.leader(slot or start))(roundSystem.leader(round)): mencius/Acceptor.scala:215-218,
    // :250-253
    def nackTo(slot: Int, round: Int, nack: Nack): Unit =
      leaders(slotSystem.leader(slot))(roundSystem.leader(round)).send(LeaderInbound().withNack(nack))
    val reply: engine.InboxReply => Unit = inbound.request match {
      case AcceptorInbound.Request.Phase1A(_) =>
        val leader = chan[Leader[Transport]](src, Leader.serializer)
        ({
          case engine.Nacked(nack)      => leader.send(LeaderInbound().withNack(nack))        // :173-180
          case engine.Promised(phase1b) => leader.send(LeaderInbound().withPhase1B(phase1b))  // :184-199
          case other                    => logger.fatal(s"Phase1a answered with $other")
        })
      case AcceptorInbound.Request.Phase2A(p) =>
        ({
          case engine.Nacked(nack) => nackTo(p.slot, p.round, nack)                           // :210-218
          case engine.Voted(phase2b) =>                                                       // :226-234
            chan[ProxyLeader[Transport]](src, ProxyLeader.serializer).send(ProxyLeaderInbound().withPhase2B(phase2b))
          case other => logger.fatal(s"Phase2a answered with $other")
        })
      case AcceptorInbound.Request.Phase2ANoopRange(p) =>
        ({
          case engine.Nacked(nack) => nackTo(p.slotStartInclusive, p.round, nack)             // :245-256
          case engine.VotedRange(phase2b) =>                                                  // :279-290
            chan[ProxyLeader[Transport]](src, ProxyLeader.serializer)
              .send(ProxyLeaderInbound().withPhase2BNoopRange(phase2b))
          case other => logger.fatal(s"Phase2aNoopRange answered with $other")
        })
      case AcceptorInbound.Request.Empty =>
        logger.fatal("Empty AcceptorInbound encountered.")
    }
    if (engine.enqueueInbox(leaderGroup, acceptorGroup, index, inbound.request, reply)) inboxTick.start()
  }

  private def receivePhase1Only(src: Transport#Address, inbound: AcceptorInbound): Unit = {
    inbound.request match {
      case AcceptorInbound.Request.Phase1A(phase1a) =>
        // enqueued, not answered: the burst a new leader sends is flushed by one tick (engine.flushPhase1as)
        val leader = chan[Leader[Transport]](src, Leader.serializer)
        val reply: Either[Nack, Phase1b] => Unit = {
          case Left(nack)     => leader.send(LeaderInbound().withNack(nack))        // mencius/Acceptor.scala:173-180
          case Right(phase1b) => leader.send(LeaderInbound().withPhase1B(phase1b))  // :184-199
        }
        if (engine.enqueuePhase1a(leaderGroup, acceptorGroup, index, phase1a, reply)) phase1Tick.start()
      case AcceptorInbound.Request.Phase2A(_) | AcceptorInbound.Request.Phase2ANoopRange(_) =>
        // the reference's leaders send these to PROXY LEADERS (mencius/Leader.scala:342-345, 455); a deployment that
        // points them at GpuMenciusProxyLeader never delivers one here
        logger.fatal("GpuMenciusAcceptor: Phase2a / Phase2aNoopRange go to GpuMenciusProxyLeader in this deployment.")
      case AcceptorInbound.Request.Empty =>
        logger.fatal("Empty AcceptorInbound encountered.")
    }
  }
}
