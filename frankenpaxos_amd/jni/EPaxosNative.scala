// EPaxosNative.scala -- the EPaxos part of the reference-side binding (source only, like Native.scala: no JDK / scalac in
// this image).  Drop into jvm/src/main/scala/frankenpaxos/gpu/ next to Native.scala.
//
//   GpuEPaxosEngine    ONE libfpx EPaxos context = the conflict indices and command logs of ALL n replicas, for a
//                      deployment whose replicas run in one process on the GPU box (one Transport event loop).
//   GpuEPaxosReplica   stands at ONE replica address (epaxos/ReplicaMain.scala); every replica address gets one, all over
//                      the same engine.  `receive` (epaxos/Replica.scala:1081-1119) only enqueues; one zero-delay
//                      Transport timer per burst flushes the queue, one native call per kind of message:
//                        ClientRequest  -> a pre-accept tick (Native.epxPreaccept: transitionToPreAcceptPhase at the
//                                          leaders, handlePreAccept at the others, handlePreAcceptOk -- K5), then
//                                          Native.epxAccept for the commands that took the slow path (K6), then Commit
//                        PreAccept      -> Native.epxHandlePreaccept (K7: a re-sent PreAccept, a recovering replica's)
//                        Accept         -> Native.epxAccept           Prepare -> Native.epxPrepare
//                      and `send`s what the Scala handlers would have sent.  Between hosted replicas nothing crosses the
//                      transport: the PreAccept / PreAcceptOk / Accept / AcceptOk of a tick are the kernels' own traffic.
//
//                      remotePeers = true (off by default; the engine created with leaderState = true): the actor LEADS
//                      its instances among replicas in OTHER processes, reference Replicas included.  A ClientRequest goes
//                      through Native.epxLead (transitionToPreAcceptPhase at this replica alone) and the PreAccept out to
//                      thriftyOtherReplicas(fastQuorumSize - 1); PreAcceptOk / AcceptOk / Nack are enqueued, and a tick
//                      flushes them through ONE Native.epxLeaderReplies call, after which Commit goes to the other
//                      replicas or Accept to slowQuorumSize - 1 of them.  The actor keeps the defaultToSlowPath and resend
//                      timers (a fired defaultToSlowPath timer becomes a kind-3 event of the next burst).  Without
//                      originateRecovery there is no Preparing phase:
//                      recovery is answered but not originated (a Nack that asks for it, outcome 6, is logged).
//
//                      originateRecovery = true (off by default; with remotePeers, the engine created with recovery = true):
//                      the actor ORIGINATES an instance's recovery.  A Nack that asks for it (outcome 6) and an instance that
//                      blocks execution start the reference's recover-instance timer (:1066, 1623-1629, 891-895); when it
//                      fires, Native.epxRecover is transitionToPreparePhase at this replica with its own Prepare, and the
//                      Prepare goes to slowQuorumSize - 1 others.  PrepareOks are enqueued and a tick flushes them through
//                      ONE Native.epxRecoveryReplies call; its decisions are applied in the same flush with Native.epxLead
//                      (avoidFastPath) or Native.epxLeadAccept, and the PreAccept or Accept is sent.  The actor keeps the
//                      resend-Prepares timer.
//
//                      inboxBurst = true (off by default): what replicas OUTSIDE send this one -- PreAccept, Accept, Prepare,
//                      Commit -- is enqueued as it arrives and a tick flushes it through ONE Native.epxReplicaInbox call, in
//                      arrival order: a leader's PreAccept that lands twice in one burst is answered twice, and an Accept is
//                      handleAccept at this replica alone (no proposer step on the hosted context, no commit on one AcceptOk).
//
// The same natives driven on wire bytes -- two conflicting commands met in different orders, differing PreAcceptOks, the
// slow path, Accept, AcceptOk, Commit -- against the oracle: tests/test_jni_shim.py::test_an_epaxos_slow_path_commit_...
//
// Execution (round 5; ADVICE r04): a committed instance goes through the reference's OWN classes -- a
// frankenpaxos.depgraph.DependencyGraph[Instance, Int, InstancePrefixSet] (the one ReplicaMain builds, :127), a
// frankenpaxos.statemachine.StateMachine and a frankenpaxos.clienttable.ClientTable per actor, exactly as
// Replica.commit / execute / executeCommand use them (:859-960): every hosted replica executes every commit, the
// instance's leader answers the client (:951-960), a request whose answer is in the client table is answered from it
// (:1121-1147).  A Commit from a replica outside is recorded in the device's command log and conflict index
// (Native.epxHandleCommit: Replica.handleCommit :1567-1575) and executed like the others.
//
// Scope (DESIGN.md section 8): get / set commands of the key-value store with any number of keys
// (statemachine/KeyValueStore.scala:221-302; a burst whose commands all have one key takes the single-key natives, any
// other burst their multi-key forms Native.epx*Mk; only KeyValueStoreInput.Request.Empty is fatal), top-one dependencies, sequence number 0; the leader-side recovery timers (Replica.scala:1021-1078) stay with a
// reference Replica if one is wanted -- Prepare / PrepareOk are answered here, not originated; the answers carry what
// the reference's handlePrepareOk reads (:1819-1843: sequenceNumber and dependencies of a PreAccepted / Accepted entry,
// the Commit for a committed one, Replica.nullBallot for an instance never seen).  `leaderStates` (the
// instances a replica is leading, :1243-1249 "stop leading when a larger ballot arrives") is empty between two bursts
// here by construction: an instance this actor leads is pre-accepted, accepted if need be and committed inside the
// flush that proposed it (flushTick checks the f + 1 votes), so a PreAccept in a larger ballot for it finds a
// CommittedEntry and is answered with the Commit (:1228-1238, K7) -- there is no leader state or timer left to drop.
package frankenpaxos.gpu

import com.google.protobuf.ByteString
import frankenpaxos.Actor
import frankenpaxos.Logger
import frankenpaxos.clienttable.ClientTable
import frankenpaxos.depgraph.DependencyGraph
import frankenpaxos.epaxos._
import frankenpaxos.statemachine.{GetRequest, KeyValueStoreInput, SetRequest, StateMachine}
import scala.collection.mutable

class GpuEPaxosEngine[Transport <: frankenpaxos.Transport[Transport]](
    logger: Logger,
    config: Config[Transport],
    numKeys: Int = 1 << 10,
    numInstances: Int = 1 << 20,         // instances (leader, number < numInstances) the command logs hold
    leaderState: Boolean = false,        // also keep Replica.leaderStates on the device (GpuEPaxosReplica's remotePeers)
    recovery: Boolean = false,           // ... with the Preparing phase (GpuEPaxosReplica's originateRecovery); needs leaderState
    deviceKeys: Boolean = false,         // key strings -> key ids in the DEVICE's table (Native.epxKeysEnable); keyOf caches it
    keyArenaBytes: Long = 1L << 24,      // ... with this many bytes for the key strings
    deviceCommands: Boolean = false,     // triple id -> command bytes in the DEVICE's store too (Native.epxCmdsEnable); needs deviceKeys
    maxDeviceTriples: Int = 1 << 22,     // ... for the triple ids below this
    commandArenaBytes: Long = 1L << 28   // ... with this many bytes for the commands
) {
  val n: Int = config.n
  val hasLeaderState: Boolean = leaderState
  val hasRecovery: Boolean = leaderState && recovery
  val hasDeviceKeys: Boolean = deviceKeys
  val handle: Long = if (hasRecovery) Native.epxCreateWithRecovery(n, numKeys, 0, numInstances)
                     else if (leaderState) Native.epxCreateWithLeaderState(n, numKeys, 0, numInstances)
                     else Native.epxCreateWithLog(n, numKeys, 0, numInstances)
  if (handle < 0) Native.check((-handle).toInt, logger)

  // a command's triple id is its index here (the GPU carries the int32; Accept and Commit name a triple by it)
  val triples = mutable.ArrayBuffer[CommandOrNoop]()
  // originateRecovery: equal commands get equal triple ids (handlePrepareOk compares the commands of PrepareOks, :1845)
  private val internedTriples = mutable.Map[CommandOrNoop, Int]()
  def intern(c: CommandOrNoop): Int = internedTriples.getOrElseUpdate(c, { triples += c; triples.size - 1 })
  // instance -> the dependencies it committed with: n watermarks + the end of the own column's explicit ids (0 = none)
  val depsOf = mutable.Map[(Int, Int), (Array[Int], Int)]()
  // triple id -> the dependencies an Accept carried (the device names an accepted triple by its id alone)
  val tripleDeps = mutable.Map[Int, (Array[Int], Int)]()
  // the actors over this engine: what one of them commits inside its flush the others learn here, not over the transport
  val actors = mutable.Buffer[GpuEPaxosReplica[Transport]]()
  val nextNumber: Array[Int] = Array.fill(n)(0)             // Replica.nextAvailableInstance, per hosted leader
  private val keyIds = mutable.Map[String, Int]()
  if (deviceKeys) Native.check(Native.epxKeysEnable(handle, keyArenaBytes), logger)
  // deviceCommands: the device keeps the triples' bytes as well, so the bytes tick encodes the Commit sent back and the
  // PrepareOk of a seen instance itself.  The ticks put the commands of the frames they decode; every other triple id -- the
  // ones leadRequests, intern and the recovery path hand to Native.epxLead* -- is put from `triples` here, before the next
  // bytes tick could be asked for it.  The ids a bytes tick carries itself (`inTick`) are left to the tick's own put, so no
  // command goes down twice; if that tick is refused the caller puts them after all (putTriples).
  logger.check(!deviceCommands || deviceKeys)
  val hasDeviceCommands: Boolean = deviceCommands
  if (deviceCommands) Native.check(Native.epxCmdsEnable(handle, maxDeviceTriples, commandArenaBytes), logger)
  private var triplesPut = 0
  var maxCommandBytes = 0                                    // the longest command put so far: sizes the bytes tick's output
  def putTriples(ids: Array[Int]): Unit = if (deviceCommands && ids.nonEmpty) {
    val cmds = ids.map(t => triples(t).toByteArray)
    val off = cmds.scanLeft(0L)(_ + _.length)
    val bytes = new Array[Byte](off.last.toInt)
    for ((c, i) <- cmds.zipWithIndex) Array.copy(c, 0, bytes, off(i).toInt, c.length)
    val result = new Array[Long](4)
    Native.check(Native.epxCmdsPut(handle, ids.length, bytes, off.last, off.init, cmds.map(_.length), ids, result), logger)
    // neither is an error of the call, but the replies of these triples stay deferred (built here) from now on: say so
    if (result(2) > 0) logger.warn(s"GpuEPaxosEngine: ${result(2)} commands skipped by the device store (id >= $maxDeviceTriples or longer than 65536 bytes)")
    if (result(3) != 0) logger.warn(s"GpuEPaxosEngine: the device command store is full ($commandArenaBytes bytes): ${ids.length} commands not stored")
    maxCommandBytes = math.max(maxCommandBytes, cmds.map(_.length).max)
  }
  def putNewTriples(inTick: Set[Int] = Set.empty): Unit = if (deviceCommands && triplesPut < triples.size) {
    putTriples((triplesPut until triples.size).filterNot(inTick).toArray)
    triplesPut = triples.size
  }
  def noteTickCommands(longest: Int): Unit = maxCommandBytes = math.max(maxCommandBytes, longest)
  // deviceKeys: the device hands out the ids (fpx_epx_keys_intern), also to the frames that go to Native.epxWireReplicaTick
  // as bytes; a miss here asks it and caches the answer, so the JVM and the device never hand out ids side by side
  private def deviceKeyOf(k: String): Int = {
    val bytes = k.getBytes(java.nio.charset.StandardCharsets.UTF_8)
    val id = new Array[Int](1)
    Native.check(Native.epxKeysIntern(handle, 1, bytes, bytes.length.toLong, Array(0L), Array(bytes.length), id), logger)
    id(0)
  }
  def keyOf(k: String): Int =
    if (deviceKeys) keyIds.getOrElseUpdate(k, deviceKeyOf(k))
    else keyIds.getOrElseUpdate(k, { logger.check(keyIds.size < numKeys); keyIds.size })

  // A caller that holds raw ReplicaInbound frames routes them by the outer oneof tag, one byte: 0x12 (PreAccept), 0x22
  // (Accept), 0x32 (Commit) and 0x3a (Prepare) go to the replica tick native (Native.scala; needs deviceKeys) as 0x1a /
  // 0x2a / 0x4a go to the leader tick native (INTEGRATION.md); every other frame, and a frame either tick refuses, is the JVM's
  def isReplicaTickFrame(first: Byte): Boolean = first == 0x12 || first == 0x22 || first == 0x32 || first == 0x3a

  // (key ids, is set) of a key-value-store command, any number of keys (KeyValueStore.scala:221-302 merges and puts over
  // all of them); only a request that is neither a get nor a set is outside the device's conflict model
  def classify(c: Command): (Array[Int], Boolean) =
    KeyValueStoreInput.parseFrom(c.command.toByteArray).request match {
      case KeyValueStoreInput.Request.GetRequest(GetRequest(keys))               => (keys.map(keyOf).toArray, false)
      case KeyValueStoreInput.Request.SetRequest(SetRequest(kvs))                => (kvs.map(kv => keyOf(kv.key)).toArray, true)
      case _ => logger.fatal("GpuEPaxosEngine: get / set commands of the key-value store only (Request.Empty).")
    }
  // the same for a triple's commandOrNoop: a Noop has no keys to put (None)
  def classify(c: CommandOrNoop): (Option[Array[Int]], Boolean) =
    if (c.value.isNoop) (None, false) else { val (k, s) = classify(c.getCommand); (Some(k), s) }

  // A burst goes to the natives it has always gone to when every command has exactly one key (key -1 = Noop); any other
  // burst takes the multi-key natives (Native.epx*Mk), which take the keys as keyOffsets (m + 1) + keys -- a Noop is an
  // empty list there, which the device treats exactly like a Noop (no dependencies, nothing put).
  def singleKeys(ks: Seq[Option[Array[Int]]]): Boolean = ks.forall(_.forall(_.length == 1))
  def singleKey(ks: Seq[Option[Array[Int]]]): Array[Int] = ks.map(_.map(_(0)).getOrElse(-1)).toArray
  def keyOffsets(ks: Seq[Option[Array[Int]]]): Array[Int] = ks.scanLeft(0)(_ + _.map(_.length).getOrElse(0)).toArray
  def keyList(ks: Seq[Option[Array[Int]]]): Array[Int] = ks.flatMap(_.getOrElse(Array.empty[Int])).toArray

  def close(): Unit = Native.check(Native.epxDestroy(handle), logger)
}

class GpuEPaxosReplica[Transport <: frankenpaxos.Transport[Transport]](
    address: Transport#Address,
    transport: Transport,
    logger: Logger,
    config: Config[Transport],
    engine: GpuEPaxosEngine[Transport],
    // what epaxos/ReplicaMain.scala hands a Replica (:120-135): this replica's copy of the state machine and its graph
    stateMachine: StateMachine,
    dependencyGraph: DependencyGraph[Instance, Int, InstancePrefixSet],
    // true: committed instances are ordered by libfpx's device dependency graph (Native.epxExecute, 2.2 - 2.6e9 commands/s
    // at 2^20 instances per call, profiles/r06_depgraph_dev.md) instead of `dependencyGraph` (the reference's, 2 - 3e7/s);
    // the state machine, the client table and the replies stay where they are.  Default off: the reference's own graph.
    deviceExecution: Boolean = false,
    // true: the other replicas live in other processes; this actor leads its instances through Native.epxLead /
    // Native.epxLeaderReplies (the engine needs leaderState = true).  Default off: all n replicas in this process.
    remotePeers: Boolean = false,
    // true: what replicas outside send this one -- PreAccept, Accept, Prepare, Commit -- goes through ONE
    // Native.epxReplicaInbox call per flush, in arrival order, instances repeated freely.
    // Default off: one native call per kind of message, as below.
    inboxBurst: Boolean = false,
    // true (needs remotePeers and an engine with recovery = true): this actor originates an instance's recovery through
    // Native.epxRecover / Native.epxRecoveryReplies / Native.epxLeadAccept.  Default off: recovery is answered only.
    originateRecovery: Boolean = false,
    prepareOksAsIntended: Boolean = false,   // handlePrepareOk's two tests as the reference's comments describe them (include/fpx.h)
    recoverInstanceTimerMinPeriod: java.time.Duration = java.time.Duration.ofMillis(500),
    recoverInstanceTimerMaxPeriod: java.time.Duration = java.time.Duration.ofMillis(1500),
    thrifty: Boolean = true,             // PreAccept / Accept to a thrifty quorum (else to every other replica)
    resendPeriod: java.time.Duration = java.time.Duration.ofSeconds(1),              // resendPreAccepts / resendAccepts
    defaultToSlowPathPeriod: java.time.Duration = java.time.Duration.ofSeconds(1)
) extends Actor(address, transport, logger) {
  override type InboundMessage = ReplicaInbound
  override val serializer = ReplicaInboundSerializer

  private val n = config.n
  private val index = config.replicaAddresses.indexOf(address)
  logger.check(index >= 0)
  private val replicas = for (a <- config.replicaAddresses) yield chan[Replica[Transport]](a, Replica.serializer)
  engine.actors += this

  // ---- execution: Replica.commit's tail, execute and executeCommand (epaxos/Replica.scala:859-960) on the reference's classes
  implicit private val addressSerializer = transport.addressSerializer
  private val clientTable = ClientTable[(Transport#Address, Int), Array[Byte]]()
  private val committed = mutable.Map[Instance, CommandOrNoop]()       // CommittedEntry.triple.commandOrNoop, until executed
  private val executables = mutable.Buffer[Instance]()
  private val blockers = mutable.Set[Instance]()

  // every actor of the process learns every commit: from its own flush, from another hosted actor's, or from a Commit message
  // ---- deviceExecution: what this replica knows of every leader's column above its executed prefix.  The device graph
  // wants DENSE columns (include/fpx.h, fpx_epx_execute): per leader the instances first .. first + count - 1, each once,
  // everything below `first` executed.  So: executedPrefix(l) = the first number of leader l not executed here yet;
  // pendingDeps = the committed instances at or above it that are not executed (watermarks, end of the own column's
  // explicit ids); executedAbove = the ones above it that are (executed out of column order: handed in again as
  // committed -- the device puts them in the order, the actor skips them); a number in the range with no Commit yet is
  // handed in as "not committed": it and whatever reaches it wait (Replica.scala:883-917 `blockers`).
  private val executedPrefix = Array.fill(n)(0)
  private val pendingDeps = mutable.Map[Instance, (Array[Int], Int)]()
  private val executedAbove = mutable.Map[Instance, (Array[Int], Int)]()
  private def ownEnd(instance: Instance, deps: InstancePrefixSetProto): Int = {
    val v = deps.intPrefixSet(instance.replicaIndex).value
    if (v.isEmpty) 0 else v.max + 1
  }

  def learnCommit(instance: Instance, commandOrNoop: CommandOrNoop, dependencies: InstancePrefixSetProto): Unit = {
    if (committed.contains(instance)) return                            // a re-sent Commit
    if (deviceExecution) {
      if (instance.instanceNumber < executedPrefix(instance.replicaIndex) || executedAbove.contains(instance)) return
      committed(instance) = commandOrNoop
      pendingDeps(instance) = (watermarks(dependencies), ownEnd(instance, dependencies))
      return
    }
    committed(instance) = commandOrNoop
    dependencyGraph.commit(instance, 0, InstancePrefixSet.fromProto(dependencies))       // :866-868
  }
  private def executeGraphOnDevice(): Unit = {
    if (pendingDeps.isEmpty) return
    val first = executedPrefix.clone()
    val count = Array.tabulate(n)(l => {
      val known = (pendingDeps.keysIterator ++ executedAbove.keysIterator).filter(_.replicaIndex == l).map(_.instanceNumber)
      if (known.isEmpty) 0 else known.max + 1 - first(l)
    })
    val m = count.sum
    val leader = new Array[Int](m); val number = new Array[Int](m); val deps = new Array[Int](m * n); val ends = new Array[Int](m)
    val isCommitted = new Array[Byte](m)
    var i = 0
    for (l <- 0 until n; x <- first(l) until first(l) + count(l)) {
      leader(i) = l; number(i) = x
      pendingDeps.get(Instance(l, x)).orElse(executedAbove.get(Instance(l, x))) match {
        case Some((w, end)) => Array.copy(w, 0, deps, i * n, n); ends(i) = end; isCommitted(i) = 1
        case None           => ()                                        // no Commit yet: blocks what reaches it
      }
      i += 1
    }
    val order = new Array[Int](m); val component = new Array[Int](m); val counts = new Array[Int](3)
    Native.check(Native.epxExecute(engine.handle, m, n, leader, number, deps, ends, isCommitted, first, count, order, component, counts), logger)
    if (counts(2) != 0) {
      // two different closures with one sum and one 22-bit hash (probability ~2^-22 per pair: include/fpx.h): this batch
      // goes through the reference's graph, which is told what has been executed so far (DependencyGraph.updateExecuted)
      logger.warn("GpuEPaxosReplica: the device dependency graph asks for the host path; this batch runs on the reference's graph.")
      // what this replica has executed: the prefixes, and the instances above them (depgraph/DependencyGraph.scala:176-186)
      val done = InstancePrefixSet.fromWatermarks(executedPrefix.toBuffer)
      executedAbove.keysIterator.foreach(done.add)
      dependencyGraph.updateExecuted(done)
      for ((inst, (w, end)) <- pendingDeps)
        dependencyGraph.commit(inst, 0, InstancePrefixSet.fromProto(prefixSet(w, inst.replicaIndex, end, inst.instanceNumber)))
      dependencyGraph.appendExecute(None, executables, blockers)
    } else {
      for (p <- 0 until counts(0)) executables += Instance(leader(order(p)), number(order(p)))
    }
    for (inst <- executables if !executedAbove.contains(inst)) {
      committed.remove(inst) match {
        case None                => logger.fatal(s"Instance $inst is ready for execution but was never committed here.")
        case Some(commandOrNoop) => executeCommand(inst, commandOrNoop)
      }
      executedAbove(inst) = pendingDeps.remove(inst).get
    }
    if (originateRecovery) for (i <- blockers if !recoverTimers.contains(i)) recoverTimers(i) = makeRecoverInstanceTimer(i)   // :891-895
    executables.clear(); blockers.clear()
    for (l <- 0 until n) {                                               // the executed prefixes move up; what lies below them is forgotten
      while (executedAbove.remove(Instance(l, executedPrefix(l))).isDefined) executedPrefix(l) += 1
    }
  }
  def executeGraph(): Unit = {                                           // :883-917
    if (deviceExecution) { executeGraphOnDevice(); return }
    dependencyGraph.appendExecute(None, executables, blockers)
    if (originateRecovery) for (i <- blockers if !recoverTimers.contains(i)) recoverTimers(i) = makeRecoverInstanceTimer(i)   // :891-895
    for (i <- executables) {
      committed.remove(i) match {
        case None                => logger.fatal(s"Instance $i is ready for execution but was never committed here.")
        case Some(commandOrNoop) => executeCommand(i, commandOrNoop)
      }
    }
    executables.clear(); blockers.clear()
  }
  private def executeCommand(instance: Instance, commandOrNoop: CommandOrNoop): Unit = commandOrNoop.value match {   // :919-965
    case CommandOrNoop.Value.Empty   => logger.fatal("Empty CommandOrNoop.")
    case CommandOrNoop.Value.Noop(_) => ()
    case CommandOrNoop.Value.Command(Command(clientAddressBytes, clientPseudonym, clientId, command)) =>
      val clientAddress = transport.addressSerializer.fromBytes(clientAddressBytes.toByteArray)
      val clientIdentity = (clientAddress, clientPseudonym)
      clientTable.executed(clientIdentity, clientId) match {
        case ClientTable.Executed(_) => ()                               // never execute a command twice
        case ClientTable.NotExecuted =>
          val output = stateMachine.run(command.toByteArray)
          clientTable.execute(clientIdentity, clientId, output)
          if (index == instance.replicaIndex)                            // the instance's leader answers the client
            chan[Client[Transport]](clientAddress, Client.serializer).send(
              ClientInbound().withClientReply(ClientReply(clientPseudonym = clientPseudonym, clientId = clientId,
                                                          result = ByteString.copyFrom(output))))
      }
  }

  private val requests = mutable.Buffer[(Transport#Address, ClientRequest)]()
  private val preAccepts = mutable.Buffer[(Transport#Address, PreAccept)]()
  private val accepts = mutable.Buffer[(Transport#Address, Accept)]()
  private val prepares = mutable.Buffer[(Transport#Address, Prepare)]()
  private val commits = mutable.Buffer[Commit]()
  private var queued = 0
  private val tick = timer("gpuEPaxosTick", java.time.Duration.ZERO, () => {
    // (PrepareOks first, and their decisions applied, before another burst of any kind reaches the context: include/fpx.h)
    if (originateRecovery) { flushPrepareOks(); flushRecoveries() }
    if (inboxBurst) flushPeerInbox()
    flushTick()
  })
  private def enqueue[T](q: mutable.Buffer[T], x: T): Unit = { if (queued == 0) tick.start(); q += x; queued += 1 }

  override def receive(src: Transport#Address, inbound: ReplicaInbound): Unit = {
    import ReplicaInbound.Request
    inbound.request match {
      case Request.ClientRequest(r) =>
        // Replica.handleClientRequest (:1121-1147): an answer that is already in the client table is relayed, a stale
        // request ignored; everything else is led in the next flush
        clientTable.executed((src, r.command.clientPseudonym), r.command.clientId) match {
          case ClientTable.NotExecuted    => enqueue(requests, (src, r))
          case ClientTable.Executed(None) => ()
          case ClientTable.Executed(Some(output)) =>
            chan[Client[Transport]](src, Client.serializer).send(
              ClientInbound().withClientReply(ClientReply(clientPseudonym = r.command.clientPseudonym,
                                                          clientId = r.command.clientId, result = ByteString.copyFrom(output))))
        }
      case Request.PreAccept(r) if inboxBurst => enqueue(peerInbox, PeerEvent(0, src, r.instance, r.ballot, Some(r.commandOrNoop), Some(r.dependencies)))
      case Request.Accept(r) if inboxBurst => enqueue(peerInbox, PeerEvent(1, src, r.instance, r.ballot, Some(r.commandOrNoop), Some(r.dependencies)))
      case Request.Commit(r) if inboxBurst => enqueue(peerInbox, PeerEvent(2, src, r.instance, Ballot(0, 0), Some(r.commandOrNoop), Some(r.dependencies)))
      case Request.Prepare(r) if inboxBurst => enqueue(peerInbox, PeerEvent(3, src, r.instance, r.ballot, None, None))
      case Request.PreAccept(r)     => enqueue(preAccepts, (src, r))
      case Request.Accept(r)        => enqueue(accepts, (src, r))
      case Request.Prepare(r)       => enqueue(prepares, (src, r))
      case Request.Commit(r)        => enqueue(commits, r)   // from a replica outside this process (Replica.handleCommit :1567)
      case Request.PreAcceptOk(r) if remotePeers =>
        enqueue(leaderInbox, LeaderEvent(0, r.instance, r.ballot, r.replicaIndex, r.sequenceNumber, Some(r.dependencies)))
      case Request.AcceptOk(r) if remotePeers => enqueue(leaderInbox, LeaderEvent(1, r.instance, r.ballot, r.replicaIndex, 0, None))
      case Request.Nack(r) if remotePeers     => enqueue(leaderInbox, LeaderEvent(2, r.instance, r.largestBallot, index, 0, None))
      case Request.PrepareOk(r) if originateRecovery => enqueue(prepareOkInbox, r)
      case Request.PreAcceptOk(_) | Request.AcceptOk(_) | Request.PrepareOk(_) | Request.Nack(_) =>
        // replies to a leader role: between hosted replicas they never leave the device; from a replica outside, they
        // belong to a reference Replica that originated the round (see the scope note above)
        logger.debug("GpuEPaxosReplica: a reply addressed to a leader role this actor does not play.")
      case Request.Empty => logger.fatal("Empty ReplicaInbound encountered.")
    }
  }

  private def bit(r: Int): Byte = (1 << r).toByte
  private def watermarks(deps: InstancePrefixSetProto): Array[Int] = deps.intPrefixSet.map(_.watermark).toArray
  private def prefixSet(w: Array[Int], own: Int, valuesEnd: Int, number: Int): InstancePrefixSetProto =
    InstancePrefixSetProto(numReplicas = n, intPrefixSet = w.indices.map(l =>
      // the own-leader column carries the explicit ids number + 1 .. valuesEnd - 1 (dependencies.subtractOne, :582)
      frankenpaxos.compact.IntPrefixSetProto(watermark = w(l), value = if (l == own && valuesEnd > 0) (number + 1 until valuesEnd) else Seq())))

  // ---- remotePeers: the leader half.  What the device keeps is Replica.leaderStates; what stays here is what only an actor
  // can hold -- the timers of an instance being led and the messages they re-send.
  private case class LeaderEvent(kind: Int, instance: Instance, ballot: Ballot, replicaIndex: Int, sequenceNumber: Int,
                                 dependencies: Option[InstancePrefixSetProto])
  private class Leading(val ballot: Ballot, val triple: Int, var resend: Transport#Timer, var slowPath: Option[Transport#Timer])
  private val leaderInbox = mutable.Buffer[LeaderEvent]()
  private val leading = mutable.Map[Instance, Leading]()
  private def otherReplicas: Seq[Int] = (1 until n).map(d => (index + d) % n)
  private def thriftyOtherReplicas(k: Int): Seq[Int] = if (thrifty) otherReplicas.take(k) else otherReplicas   // :556-563
  private def resendTimer(name: String, msg: ReplicaInbound): Transport#Timer = {                               // :996-1013, 1038-1051
    lazy val t: Transport#Timer = timer(name, resendPeriod, () => { otherReplicas.foreach(replicas(_).send(msg)); t.start() })
    t.start()
    t
  }
  private def stopLeading(instance: Instance): Unit =                                                            // stopTimers :618-630
    leading.remove(instance).foreach { l => l.resend.stop(); l.slowPath.foreach(_.stop()) }
  // a PreAccept / Accept / Prepare of a higher ballot takes the instance away (:1239-1242, 1480-1483, 1645-1648); the device
  // sees it in the command-log entry the message moved, the timers are stopped here
  private def ballotLt(a: Ballot, b: Ballot): Boolean =
    a.ordering < b.ordering || (a.ordering == b.ordering && a.replicaIndex < b.replicaIndex)
  private def yieldTo(instance: Instance, ballot: Ballot): Unit = {
    if (leading.get(instance).exists(l => ballotLt(l.ballot, ballot))) stopLeading(instance)
    if (originateRecovery && recovering.get(instance).exists(r => ballotLt(r.ballot, ballot))) stopRecovering(instance)
  }

  // transitionToPreAcceptPhase (:633-729) of a batch of pairwise distinct instances at THIS replica: the one place that
  // calls Native.epxLead -- for ClientRequests, and for the recoveries that start over (originateRecovery).  Returns the
  // dependencies of the PreAccepts to send: (m x n watermarks, m values ends)
  private def leadHere(leader: Array[Int], number: Array[Int], ballotOrdering: Array[Int], keys: Seq[Option[Array[Int]]],
                       isSet: Array[Byte], tripleId: Array[Int], avoidFastPath: Array[Byte]): (Array[Int], Array[Int]) = {
    val m = leader.length
    val deps = new Array[Int](m * n); val ends = new Array[Int](m)
    // (engine.singleKeys: the natives this has always gone to when every command has one key, else their Mk forms)
    val st = if (engine.singleKeys(keys))
               Native.epxLead(engine.handle, m, n, leader, number, Array.fill(m)(index), ballotOrdering, engine.singleKey(keys), isSet,
                              tripleId, avoidFastPath, deps, ends)
             else
               Native.epxLeadMk(engine.handle, m, n, leader, number, Array.fill(m)(index), ballotOrdering, engine.keyOffsets(keys),
                                engine.keyList(keys), isSet, tripleId, avoidFastPath, deps, ends)
    if (st == 9) logger.fatal("transitionToPreAcceptPhase: the instance is committed or known in a larger ballot (:662-682).")
    Native.check(st, logger)
    (deps, ends)
  }

  // ClientRequests, led at THIS replica alone: transitionToPreAcceptPhase (:633-729) through Native.epxLead
  private def leadRequests(): Unit = {
    val m = requests.size
    logger.check(engine.hasLeaderState)
    val leader = Array.fill(m)(index); val number = new Array[Int](m); val isSet = new Array[Byte](m)
    val keys = new Array[Option[Array[Int]]](m)
    val first = engine.triples.size
    for (((_, r), i) <- requests.zipWithIndex) {
      number(i) = engine.nextNumber(index); engine.nextNumber(index) += 1
      val (k, set) = engine.classify(r.command)
      keys(i) = Some(k); isSet(i) = if (set) 1 else 0
      engine.triples += CommandOrNoop().withCommand(r.command)
    }
    val (deps, ends) = leadHere(leader, number, Array.fill(m)(0), keys, isSet, Array.tabulate(m)(first + _), new Array[Byte](m))
    val ballot = Ballot(0, index)                                                                               // defaultBallot :453
    for (i <- 0 until m) {
      val instance = Instance(index, number(i))
      val preAccept = ReplicaInbound().withPreAccept(PreAccept(instance = instance, ballot = ballot,
        commandOrNoop = engine.triples(first + i), sequenceNumber = 0,
        dependencies = prefixSet(deps.slice(i * n, (i + 1) * n), index, ends(i), number(i))))
      thriftyOtherReplicas(config.fastQuorumSize - 1).foreach(replicas(_).send(preAccept))                      // :705-706
      leading(instance) = new Leading(ballot, first + i, resendTimer(s"resendPreAccepts $instance $ballot", preAccept), None)
    }
    requests.clear()
  }

  // the burst's PreAcceptOks, AcceptOks, Nacks and fired defaultToSlowPath timers: ONE device call, then what the handlers
  // would have sent
  private def flushLeaderReplies(): Unit = {
    val k = leaderInbox.size
    val ev = leaderInbox.toArray
    val zeros = Array.fill(n)(0)
    val deps = ev.flatMap(e => e.dependencies.map(watermarks).getOrElse(zeros))
    val ends = ev.map(e => e.dependencies.map(d => ownEnd(e.instance, d)).getOrElse(0))
    val outcome = new Array[Int](k); val triple = new Array[Int](3 * k); val outDeps = new Array[Int](k * n)
    val decided = new Array[Int](k + 1)
    val st = Native.epxLeaderReplies(engine.handle, k, n, ev.map(_.kind), Array.fill(k)(index), ev.map(_.instance.replicaIndex),
                                     ev.map(_.instance.instanceNumber), ev.map(_.ballot.ordering), ev.map(_.ballot.replicaIndex),
                                     ev.map(_.replicaIndex), ev.map(_.sequenceNumber), deps, ends, outcome, triple, outDeps, decided)
    leaderInbox.clear()
    if (st == 9) logger.fatal("a reply in a ballot above the one led in (logger.checkLt :1333, :1550), or a defaultToSlowPath " +
                              "timer outside the pre-accept phase (:1024-1028).")
    Native.check(st, logger)
    for (i <- 0 until k) outcome(i) match {
      case 2 =>                                                                                                 // :1353-1364
        val instance = ev(i).instance
        leading.get(instance).foreach { l =>
          val t = timer(s"defaultToSlowPath $instance", defaultToSlowPathPeriod,
                        () => enqueue(leaderInbox, LeaderEvent(3, instance, l.ballot, index, 0, None)))
          t.start(); l.slowPath = Some(t)
        }
      case 6 if originateRecovery => startOrResetRecoverTimer(ev(i).instance)                                   // :1623-1629
      case 6 => logger.debug(s"GpuEPaxosReplica: Nack for ${ev(i).instance} in a larger ballot; recovery is not originated here.")
      case _ => ()
    }
    for (j <- 1 to decided(0)) {
      val i = decided(j)
      val instance = ev(i).instance
      val (l, x) = (instance.replicaIndex, instance.instanceNumber)
      val w = outDeps.slice(i * n, (i + 1) * n); val end = triple(k + i); val id = triple(2 * k + i)
      val dependencies = prefixSet(w, l, end, x)
      if (outcome(i) == 4) {                                                                                    // transitionToAcceptPhase :765-792
        leading.get(instance).foreach { led =>
          led.resend.stop(); led.slowPath.foreach(_.stop()); led.slowPath = None
          val accept = ReplicaInbound().withAccept(Accept(instance = instance, ballot = led.ballot, commandOrNoop = engine.triples(id),
                                                          sequenceNumber = triple(i), dependencies = dependencies))
          thriftyOtherReplicas(config.slowQuorumSize - 1).foreach(replicas(_).send(accept))
          led.resend = resendTimer(s"resendAccepts $instance ${led.ballot}", accept)
        }
        engine.tripleDeps(id) = (w, end)
      } else {                                                                                                  // commit :815-860
        stopLeading(instance)
        engine.depsOf((l, x)) = (w, end)
        val commit = Commit(instance = instance, commandOrNoop = engine.triples(id), sequenceNumber = triple(i), dependencies = dependencies)
        otherReplicas.foreach(replicas(_).send(ReplicaInbound().withCommit(commit)))
        learnCommit(instance, commit.commandOrNoop, commit.dependencies)
      }
    }
    if (decided(0) > 0) executeGraph()
  }

  // ---- originateRecovery: the Preparing phase.  The device keeps the Preparing state and its PrepareOks; what stays here
  // is the recover-instance timers (:513, 1066-1078), the resend-Prepares timer of an instance being recovered (:1053-1064)
  // and the interned commands the PrepareOks named.
  private val prepareOkInbox = mutable.Buffer[PrepareOk]()
  private val recoverTimers = mutable.Map[Instance, Transport#Timer]()
  private class Recovering(val ballot: Ballot, val resend: Transport#Timer)
  private val recovering = mutable.Map[Instance, Recovering]()
  private val toRecover = mutable.Buffer[Instance]()
  private val noopTriple: Int = if (originateRecovery) engine.intern(CommandOrNoop().withNoop(Noop())) else -1
  logger.check(!originateRecovery || (remotePeers && engine.hasRecovery))
  private def makeRecoverInstanceTimer(instance: Instance): Transport#Timer = {                                  // :1066-1078
    lazy val t: Transport#Timer = timer(s"recoverInstance $instance",
      frankenpaxos.Util.randomDuration(recoverInstanceTimerMinPeriod, recoverInstanceTimerMaxPeriod),
      () => { enqueue(toRecover, instance); t.start() })
    t.start()
    t
  }
  private def startOrResetRecoverTimer(instance: Instance): Unit = recoverTimers.get(instance) match {
    case Some(t) => t.reset()
    case None    => recoverTimers(instance) = makeRecoverInstanceTimer(instance)
  }
  // handlePreAccept / handleAccept / handlePrepare reset it (:1249, 1490, 1640); commit stops it (:849-856)
  private def resetRecoverTimer(instance: Instance): Unit = recoverTimers.get(instance).foreach(_.reset())
  private def stopRecoverTimer(instance: Instance): Unit = recoverTimers.remove(instance).foreach(_.stop())
  private def stopRecovering(instance: Instance): Unit = recovering.remove(instance).foreach(_.resend.stop())

  // the recover-instance timers that fired since the last flush: transitionToPreparePhase (:969-996) at this replica, with
  // its own Prepare, in ONE device call; then the Prepare to slowQuorumSize - 1 others
  private def flushRecoveries(): Unit = {
    val inst = toRecover.distinct.toArray                              // (the instances of one call are pairwise distinct)
    toRecover.clear()
    val m = inst.length
    if (m == 0) return
    val result = new Array[Int](5 * m)
    val st = Native.epxRecover(engine.handle, m, n, inst.map(_.replicaIndex), inst.map(_.instanceNumber), Array.fill(m)(index), result)
    if (st == 9) logger.fatal("transitionToPreparePhase: an entry in a ballot not below largestBallot + 1.")
    Native.check(st, logger)
    for (i <- 0 until m if result(i) == 0) {                           // (1: committed here -- the Commit went round already)
      val instance = inst(i)
      stopLeading(instance); stopRecovering(instance)                  // :970 stopTimers(instance)
      val ballot = Ballot(result(m + i), index)
      val prepare = ReplicaInbound().withPrepare(Prepare(instance = instance, ballot = ballot))
      thriftyOtherReplicas(config.slowQuorumSize - 1).foreach(replicas(_).send(prepare))                          // :978-983
      recovering(instance) = new Recovering(ballot, resendTimer(s"resendPrepares $instance $ballot", prepare))
    }
  }

  // the burst's PrepareOks: ONE device call (handlePrepareOk :1759-1869), and its decisions applied before anything else
  // reaches the context -- between the two calls the device holds no state for the instance
  private def flushPrepareOks(): Unit = {
    val k = prepareOkInbox.size
    if (k == 0) return
    val ev = prepareOkInbox.toArray
    prepareOkInbox.clear()
    val zeros = Array.fill(n)(0)
    val status = ev.map(_.status match { case CommandStatus.NotSeen => 0; case CommandStatus.PreAccepted => 2; case _ => 3 })
    val nul = (b: Ballot) => b.ordering < 0
    val tripleId = ev.map(e => e.commandOrNoop.map(engine.intern).getOrElse(-1))
    val deps = ev.zip(status).flatMap { case (e, s) => if (s == 0) zeros else e.dependencies.map(watermarks).getOrElse(zeros) }
    val ends = ev.zip(status).map { case (e, s) => if (s == 0) 0 else e.dependencies.map(d => ownEnd(e.instance, d)).getOrElse(0) }
    val outcome = new Array[Int](k); val decision = new Array[Int](5 * k); val outDeps = new Array[Int](k * n)
    val decided = new Array[Int](k + 1)
    val st = Native.epxRecoveryReplies(engine.handle, k, n, Array.fill(k)(index), ev.map(_.instance.replicaIndex),
                                       ev.map(_.instance.instanceNumber), ev.map(_.ballot.ordering), ev.map(_.ballot.replicaIndex),
                                       ev.map(_.replicaIndex), status, ev.map(e => if (nul(e.voteBallot)) -1 else e.voteBallot.ordering),
                                       ev.map(e => if (nul(e.voteBallot)) -1 else e.voteBallot.replicaIndex), tripleId,
                                       ev.map(_.sequenceNumber.getOrElse(0)), deps, ends, if (prepareOksAsIntended) 1 else 0,
                                       outcome, decision, outDeps, decided)
    if (st == 9) logger.fatal("a PrepareOk in a ballot above the one recovered in (logger.checkLt :1792).")
    Native.check(st, logger)
    val d = (1 to decided(0)).map(decided(_))
    val (toAccept, toLead) = d.partition(outcome(_) == 2)
    val ballotOf = (i: Int) => Ballot(decision(2 * k + i) >> 3, decision(2 * k + i) & 7)
    d.foreach(i => stopRecovering(ev(i).instance))
    if (toLead.nonEmpty) {                                             // :1856-1867 transitionToPreAcceptPhase, avoidFastPath
      val m = toLead.size
      val id = toLead.map(i => if (outcome(i) == 4) noopTriple else decision(k + i)).toArray
      val cls = id.map(t => engine.classify(engine.triples(t)))
      val (lDeps, lEnds) = leadHere(toLead.map(ev(_).instance.replicaIndex).toArray, toLead.map(ev(_).instance.instanceNumber).toArray,
                                    toLead.map(ballotOf(_).ordering).toArray, cls.map(_._1),
                                    cls.map(c => (if (c._2) 1 else 0).toByte), id, Array.fill(m)(1.toByte))
      for ((i, j) <- toLead.zipWithIndex) {
        val instance = ev(i).instance
        val preAccept = ReplicaInbound().withPreAccept(PreAccept(instance = instance, ballot = ballotOf(i),
          commandOrNoop = engine.triples(id(j)), sequenceNumber = 0,
          dependencies = prefixSet(lDeps.slice(j * n, (j + 1) * n), instance.replicaIndex, lEnds(j), instance.instanceNumber)))
        thriftyOtherReplicas(config.fastQuorumSize - 1).foreach(replicas(_).send(preAccept))
        leading(instance) = new Leading(ballotOf(i), id(j), resendTimer(s"resendPreAccepts $instance ${ballotOf(i)}", preAccept), None)
      }
    }
    if (toAccept.nonEmpty) {                                           // :1813-1851 transitionToAcceptPhase with the triple
      val m = toAccept.size
      val id = toAccept.map(i => decision(k + i)).toArray
      val cls = id.map(t => engine.classify(engine.triples(t)))
      val aKeys = cls.map(_._1).toSeq; val aSet = cls.map(c => (if (c._2) 1 else 0).toByte)
      val (aLeader, aNumber) = (toAccept.map(ev(_).instance.replicaIndex).toArray, toAccept.map(ev(_).instance.instanceNumber).toArray)
      val aDeps = toAccept.flatMap(i => outDeps.slice(i * n, (i + 1) * n)).toArray
      val aEnds = toAccept.map(i => decision(4 * k + i)).toArray; val aSeq = toAccept.map(i => decision(3 * k + i)).toArray
      val aOrd = toAccept.map(ballotOf(_).ordering).toArray
      val st2 = if (engine.singleKeys(aKeys))
                  Native.epxLeadAccept(engine.handle, m, n, aLeader, aNumber, Array.fill(m)(index), aOrd, engine.singleKey(aKeys), aSet,
                                       id, aSeq, aDeps, aEnds)
                else
                  Native.epxLeadAcceptMk(engine.handle, m, n, aLeader, aNumber, Array.fill(m)(index), aOrd, engine.keyOffsets(aKeys),
                                         engine.keyList(aKeys), aSet, id, aSeq, aDeps, aEnds)
      if (st2 == 9) logger.fatal("transitionToAcceptPhase: the instance is committed or known in a larger ballot (:740-757).")
      Native.check(st2, logger)
      for ((i, j) <- toAccept.zipWithIndex) {
        val instance = ev(i).instance
        val (l, x) = (instance.replicaIndex, instance.instanceNumber)
        // the triple's dependencies: the PrepareOk's, or -- the own entry knew its triple by id alone -- the engine's
        val (w, end) = if (aDeps(j * n) >= 0) (aDeps.slice(j * n, (j + 1) * n), aEnds(j))
                       else engine.tripleDeps.getOrElse(id(j), (Array.fill(n)(0), 0))
        engine.tripleDeps(id(j)) = (w, end)
        val accept = ReplicaInbound().withAccept(Accept(instance = instance, ballot = ballotOf(i), commandOrNoop = engine.triples(id(j)),
                                                        sequenceNumber = aSeq(j), dependencies = prefixSet(w, l, end, x)))
        thriftyOtherReplicas(config.slowQuorumSize - 1).foreach(replicas(_).send(accept))
        leading(instance) = new Leading(ballotOf(i), id(j), resendTimer(s"resendAccepts $instance ${ballotOf(i)}", accept), None)
      }
    }
  }

  // ---- inboxBurst: the replica half.  What replicas outside sent since the last flush -- PreAccepts, Accepts, Commits,
  // Prepares, in arrival order -- goes through ONE device call (fpx_epx_replica_inbox), which answers every message as
  // handlePreAccept / handleAccept / handleCommit / handlePrepare would one at a time; then what the handlers would have sent.
  private case class PeerEvent(kind: Int, src: Transport#Address, instance: Instance, ballot: Ballot,
                               commandOrNoop: Option[CommandOrNoop], dependencies: Option[InstancePrefixSetProto])
  private val peerInbox = mutable.Buffer[PeerEvent]()
  // the own-leader column as the device's command log holds it: (watermark <= number, explicit ids number + 1 .. end - 1)
  private def deviceShape(instance: Instance, deps: InstancePrefixSetProto): Boolean = {
    val own = deps.intPrefixSet(instance.replicaIndex)
    val x = instance.instanceNumber
    own.value.isEmpty || (own.watermark <= x && own.value.sorted == (x + 1 to own.value.max))
  }
  // The burst through Native.epxWireReplicaTickBytes (include/fpx_wire.h, fpx_wire_epx_replica_tick_bytes): the device decodes
  // the frames, interns the keys, answers the burst and serialises the replies.  The result: per message the bytes to send
  // back, null where there is nothing to send or the reply is deferred to the loop in flushPeerInbox (which reads outcome /
  // reply / outDeps, filled here as epxReplicaInboxMk fills them).  null altogether: the tick refused a frame, nothing was
  // applied.  (The actor framework hands this actor parsed messages, so the frames are serialised again here; a transport
  // that hands over the raw frames passes them straight through, INTEGRATION.md.)
  private def wireTickBytes(ev: Array[PeerEvent], tripleId: Array[Int], outcome: Array[Int], reply: Array[Int],
                            outDeps: Array[Int]): Array[Array[Byte]] = {
    val k = ev.length
    val frames: Array[Array[Byte]] = ev.map(e => (e.kind match {
      case 0 => ReplicaInbound().withPreAccept(PreAccept(e.instance, e.ballot, e.commandOrNoop.get, 0, e.dependencies.get))
      case 1 => ReplicaInbound().withAccept(Accept(e.instance, e.ballot, e.commandOrNoop.get, 0, e.dependencies.get))
      case 2 => ReplicaInbound().withCommit(Commit(e.instance, e.commandOrNoop.get, 0, e.dependencies.get))
      case _ => ReplicaInbound().withPrepare(Prepare(e.instance, e.ballot))
    }).toByteArray)
    def direct(bytes: Int) = java.nio.ByteBuffer.allocateDirect(math.max(bytes, 8)).order(java.nio.ByteOrder.nativeOrder)
    val inLen = frames.map(_.length.toLong).sum
    val in = direct(inLen.toInt); val inOffsets = direct(8 * (k + 1)); val to = direct(4 * k)
    var at = 0L
    for ((f, i) <- frames.zipWithIndex) { inOffsets.putLong(8 * i, at); in.put(f); at += f.length; to.putInt(4 * i, index) }
    inOffsets.putLong(8 * k, at)
    // 472 * m is FPX_WIRE_EPX_REPLY_MAX: without the command store FPX_ECAPACITY cannot happen.  With it a reply may carry
    // any stored command, 503 + its bytes (FPX_WIRE_EPX_CMD_REPLY_MAX, none above 65536): the worst case where that is small,
    // else a budget of four times the burst's own bytes -- and a burst that outgrows it is answered the parsed way (below)
    val carried = (for ((e, i) <- ev.zipWithIndex if e.commandOrNoop.nonEmpty && tripleId(i) >= 0) yield tripleId(i)).toSet
    engine.putNewTriples(inTick = carried)                   // (the frames' own commands: the tick puts them)
    if (engine.hasDeviceCommands)
      engine.noteTickCommands(ev.flatMap(_.commandOrNoop).map(_.serializedSize).foldLeft(0)(math.max))
    val worst = (503L + math.min(engine.maxCommandBytes, 65536)) * k
    val outCap = if (!engine.hasDeviceCommands) 472L * k
                 else math.min(math.min(worst, 503L * k + math.max(4 * inLen, 1L << 20)), Int.MaxValue - 8L)
    val out = direct(outCap.toInt); val outOffsets = direct(8 * (k + 1)); val replyKind = direct(k)
    val result = new Array[Long](6)
    val maxPairs = math.min(frames.map(_.length).sum, 1 << 24)   // (a key is at least two bytes of its frame)
    val st = Native.epxWireReplicaTickBytes(engine.handle, k, n, in, inLen, inOffsets, to, 0, tripleId, maxPairs, out, outCap,
                                            outOffsets, replyKind, outcome, reply, outDeps, result)
    if (st == 1 && result(0) >= 0) {                         // a frame the device does not take: nothing applied, nothing interned
      engine.putTriples(carried.toArray.sorted)              // (... nor stored: the parsed way's natives put no commands)
      return null
    }
    // the encoder's FPX_ECAPACITY (result(3) > outCap): the tick WAS applied and outcome / reply / outDeps are valid, so every
    // reply of this burst is built from them as a deferred one is
    if (st == 5 && result(3) > outCap) return Array.fill[Array[Byte]](k)(null)
    Native.check(st, logger)
    Array.tabulate(k) { i =>
      if (replyKind.get(i) != 1) null
      else {
        val (lo, hi) = (outOffsets.getLong(8 * i).toInt, outOffsets.getLong(8 * (i + 1)).toInt)
        val bytes = new Array[Byte](hi - lo)
        out.position(lo); out.get(bytes); bytes
      }
    }
  }

  private def flushPeerInbox(): Unit = {
    if (peerInbox.isEmpty) return
    val k = peerInbox.size
    val ev = peerInbox.toArray
    peerInbox.clear()
    if (remotePeers) for (e <- ev) if (e.kind == 2) stopLeading(e.instance) else yieldTo(e.instance, e.ballot)
    if (originateRecovery) for (e <- ev) if (e.kind == 2) { stopRecoverTimer(e.instance); stopRecovering(e.instance) } else resetRecoverTimer(e.instance)
    val keys = Array.fill[Option[Array[Int]]](k)(None); val isSet = new Array[Byte](k); val tripleId = Array.fill(k)(-1)
    val deps = new Array[Int](k * n); val ends = new Array[Int](k)
    for ((e, i) <- ev.zipWithIndex; c <- e.commandOrNoop; d <- e.dependencies) {
      // (originateRecovery: equal commands get equal ids -- the own PrepareOk's triple id meets the peers' in handlePrepareOk)
      if (originateRecovery) tripleId(i) = engine.intern(c) else { tripleId(i) = engine.triples.size; engine.triples += c }
      val (w, end) = (watermarks(d), ownEnd(e.instance, d))
      // an Accept's or a Commit's dependencies that the command log does not represent stay here; the device names the
      // triple by its id alone (a row starting with -1).  A PreAccept's are checked by the device (FPX_EINVAL).
      if (e.kind == 0 || deviceShape(e.instance, d)) { Array.copy(w, 0, deps, i * n, n); ends(i) = end } else deps(i * n) = -1
      if (e.kind == 1) engine.tripleDeps(tripleId(i)) = (w, end)
    }
    val outcome = new Array[Int](k); val reply = new Array[Int](4 * k); val outDeps = new Array[Int](k * n)
    // deviceKeys: the burst goes down as frames and the replies come back serialised (Native.epxWireReplicaTickBytes);
    // encoded(i) is then reply i's bytes and the loop below builds only the deferred ones.  null: the tick refused a frame
    // with nothing applied (dependencies or a command outside the canonical shape), and the burst goes the parsed way
    val encoded: Array[Array[Byte]] = if (engine.hasDeviceKeys) wireTickBytes(ev, tripleId, outcome, reply, outDeps) else null
    if (encoded == null) for ((e, i) <- ev.zipWithIndex; c <- e.commandOrNoop) {
      val (ks, set) = engine.classify(c)
      keys(i) = ks; isSet(i) = if (set) 1 else 0
    }
    // (a Prepare has no command: None, which is key -1 in the one form and an empty list in the other; neither is read)
    if (encoded == null)
    Native.check(if (engine.singleKeys(keys))
                   Native.epxReplicaInbox(engine.handle, k, n, ev.map(_.kind), Array.fill(k)(index), ev.map(_.instance.replicaIndex),
                                          ev.map(_.instance.instanceNumber), ev.map(_.ballot.ordering), ev.map(_.ballot.replicaIndex),
                                          engine.singleKey(keys), isSet, tripleId, deps, ends, outcome, reply, outDeps)
                 else
                   Native.epxReplicaInboxMk(engine.handle, k, n, ev.map(_.kind), Array.fill(k)(index),
                                            ev.map(_.instance.replicaIndex), ev.map(_.instance.instanceNumber),
                                            ev.map(_.ballot.ordering), ev.map(_.ballot.replicaIndex), engine.keyOffsets(keys),
                                            engine.keyList(keys), isSet, tripleId, deps, ends, outcome, reply, outDeps), logger)
    var learnt = false
    for ((e, i) <- ev.zipWithIndex) {
      val back = chan[Replica[Transport]](e.src, Replica.serializer)
      val (l, x) = (e.instance.replicaIndex, e.instance.instanceNumber)
      val ballot = reply(i); val triple = reply(3 * k + i)
      // the reply's dependencies: from the command log, or -- a triple the device knows by its id -- from the engine
      def sent: Option[InstancePrefixSetProto] =
        (if (outDeps(i * n) >= 0) Some((outDeps.slice(i * n, (i + 1) * n), reply(2 * k + i)))
         else engine.tripleDeps.get(triple).orElse(engine.depsOf.get((l, x)))).map { case (w, end) => prefixSet(w, l, end, x) }
      if (encoded != null && encoded(i) != null) transport.send(this, e.src, encoded(i))   // the device wrote this reply
      else outcome(i) match {
        case 1 | 2 => back.send(ReplicaInbound().withPreAcceptOk(PreAcceptOk(e.instance, e.ballot, index, 0, sent.get)))   // :1196-1210, 1281-1288
        case 3 | 4 => back.send(ReplicaInbound().withAcceptOk(AcceptOk(e.instance, e.ballot, index)))                    // :1451-1461, 1505-1511
        case 5 =>                                                                                                       // :1567-1575
          val d = e.dependencies.get
          engine.depsOf((l, x)) = (watermarks(d), ownEnd(e.instance, d))
          learnCommit(e.instance, e.commandOrNoop.get, d); learnt = true
        case 6 =>                                                                                                       // :1654-1743
          val status = reply(k + i)
          val seen = status != 0 && triple >= 0
          back.send(ReplicaInbound().withPrepareOk(PrepareOk(
            ballot = e.ballot, instance = e.instance, replicaIndex = index,
            voteBallot = if (ballot < 0) Replica.nullBallot else Ballot(ballot >> 3, ballot & 7),
            status = status match { case 0 | 1 => CommandStatus.NotSeen; case 2 => CommandStatus.PreAccepted; case _ => CommandStatus.Accepted },
            commandOrNoop = if (seen) Some(engine.triples(triple)) else None,
            sequenceNumber = if (seen) Some(0) else None,
            dependencies = if (seen) sent else None)))
        case 7 => back.send(ReplicaInbound().withNack(Nack(e.instance, Ballot(ballot >> 3, ballot & 7))))
        case 8 => sent.foreach(d => back.send(ReplicaInbound().withCommit(Commit(e.instance, engine.triples(triple), 0, d))))
        case _ => ()                                                                                                    // :1222-1224
      }
    }
    if (learnt) executeGraph()
  }

  private def flushTick(): Unit = {
    if (remotePeers) {
      if (requests.nonEmpty) leadRequests()
      for (c <- commits) stopLeading(c.instance)                                                                // commit :822, :831
      for ((_, p) <- preAccepts) yieldTo(p.instance, p.ballot)
      for ((_, a) <- accepts) yieldTo(a.instance, a.ballot)
      for ((_, p) <- prepares) yieldTo(p.instance, p.ballot)
    }
    if (originateRecovery) {
      for (c <- commits) { stopRecoverTimer(c.instance); stopRecovering(c.instance) }                           // :849-856
      for ((_, p) <- preAccepts) resetRecoverTimer(p.instance)                                                  // :1249
      for ((_, a) <- accepts) resetRecoverTimer(a.instance)                                                     // :1490
      for ((_, p) <- prepares) resetRecoverTimer(p.instance)                                                    // :1640
    }
    // ---- the burst's client requests, led by THIS replica: one pre-accept tick (epaxos/Replica.scala:1121-1157,
    // 633-729, 1159-1419).  The tick's delivery order at every replica is the arrival order here; the PreAccept goes to
    // all other replicas (ThriftySystem.NotThrifty, :83), the first n - 2 answers are counted (:1376)
    val m = requests.size
    if (m > 0) {
      val leader = Array.fill(m)(index); val number = new Array[Int](m)
      val keys = new Array[Option[Array[Int]]](m); val isSet = new Array[Byte](m)
      val resp = new Array[Byte](m); val seen = new Array[Byte](m)
      val rank = Array.tabulate(n * m)(i => i % m)
      val others = (0 until n).filter(_ != index)
      val counted = others.take(n - 2).map(1 << _).sum.toByte; val all = others.map(1 << _).sum.toByte
      val first = engine.triples.size
      for (((_, r), i) <- requests.zipWithIndex) {
        number(i) = engine.nextNumber(index); engine.nextNumber(index) += 1
        val (k, set) = engine.classify(r.command); keys(i) = Some(k); isSet(i) = if (set) 1 else 0
        resp(i) = counted; seen(i) = all
        engine.triples += CommandOrNoop().withCommand(r.command)
      }
      val fast = new Array[Byte](m); val deps = new Array[Int](m * n); val ldeps = new Array[Int](m * n); val ends = new Array[Int](2 * m)
      Native.check(if (engine.singleKeys(keys))
                     Native.epxPreaccept(engine.handle, m, n, leader, number, engine.singleKey(keys), isSet, resp, seen, rank, fast,
                                         deps, ldeps, ends)
                   else
                     Native.epxPreacceptMk(engine.handle, m, n, leader, number, engine.keyOffsets(keys), engine.keyList(keys), isSet,
                                           resp, seen, rank, fast, deps, ldeps, ends), logger)
      // the slow path: Accept with the union of the answers (preAcceptingSlowPath :796-813), f other replicas + the proposer
      val slow = (0 until m).filter(fast(_) == 0).toArray
      if (slow.nonEmpty) {
        val k = slow.length
        val tgt = Array.fill(k)(others.take(config.f).map(1 << _).sum.toByte)
        val replies = new Array[Byte](4 * k); val nb = new Array[Int](k)
        val sk = slow.map(keys).toSeq
        Native.check(if (engine.singleKeys(sk))
                       Native.epxAccept(engine.handle, k, slow.map(leader), slow.map(number), Array.fill(k)(0), Array.fill(k)(index),
                                        slow.map(first + _), engine.singleKey(sk), slow.map(isSet), tgt, replies, nb)
                     else
                       Native.epxAcceptMk(engine.handle, k, slow.map(leader), slow.map(number), Array.fill(k)(0), Array.fill(k)(index),
                                          slow.map(first + _), engine.keyOffsets(sk), engine.keyList(sk), slow.map(isSet), tgt, replies,
                                          nb), logger)
        for ((i, j) <- slow.zipWithIndex) logger.check(replies(3 * k + j) != 0)   // f + 1 votes: committed (no competing ballot exists)
      }
      // commit (:815-860): every replica outside this process learns it; the hosted ones already hold the CommittedEntry
      for (i <- 0 until m) {
        val w = deps.slice(i * n, (i + 1) * n)
        engine.depsOf((index, number(i))) = (w, ends(2 * i))
        val commit = Commit(instance = Instance(index, number(i)), commandOrNoop = engine.triples(first + i), sequenceNumber = 0,
                            dependencies = prefixSet(w, index, ends(2 * i), number(i)))
        for ((a, r) <- config.replicaAddresses.zipWithIndex if !hosted(a)) replicas(r).send(ReplicaInbound().withCommit(commit))
        engine.actors.foreach(_.learnCommit(commit.instance, commit.commandOrNoop, commit.dependencies))
      }
      requests.clear()
      engine.actors.foreach(_.executeGraph())   // :869-873 with executeGraphBatchSize = the burst
    }
    // ---- Commits from replicas outside (Replica.handleCommit :1567-1575): the device's command log and conflict index at
    // THIS replica learn them (a later Prepare / PreAccept for the instance is answered with the Commit), then the graph
    if (commits.nonEmpty) {
      // The device's command log holds an instance's own-leader column as (watermark <= number, explicit ids number + 1 ..
      // end - 1): what dependencies.subtractOne(instance) makes of a cover (Replica.scala:582).  A reference Replica may send
      // any InstancePrefixSet; a Commit whose own column is not of that shape is still learnt by the graph below, but the
      // device's log does not take it -- logged and dropped there, not a fatal (ADVICE r05: input from outside is not an
      // invariant of this process).  Of several Commits for one instance in the burst the LAST one wins whole, as when the
      // reference applies them in order (the library takes care of that: fpx_epx_handle_commit).
      def deviceShape(c: Commit): Boolean = {
        val own = c.dependencies.intPrefixSet(c.instance.replicaIndex)
        val x = c.instance.instanceNumber
        own.value.isEmpty || (own.watermark <= x && own.value.sorted == (x + 1 to own.value.max))
      }
      val (forDevice, notForDevice) = commits.partition(deviceShape)
      notForDevice.foreach(c => logger.warn(s"GpuEPaxosReplica: Commit of ${c.instance} carries an own-leader column the " +
                                            "device's command log does not represent; learnt by the graph only."))
      val endsOf = mutable.Map[Commit, Int]()
      if (forDevice.nonEmpty) {
        val k = forDevice.size
        val keyset = forDevice.map(c => engine.classify(c.commandOrNoop)); val ks = keyset.map(_._1)
        val first = engine.triples.size; forDevice.foreach(c => engine.triples += c.commandOrNoop)
        val own = forDevice.map(c => c.dependencies.intPrefixSet(c.instance.replicaIndex).value)
        val endsIn = own.map(v => if (v.isEmpty) 0 else v.max + 1).toArray
        val (ls, ns, ts) = (forDevice.map(_.instance.replicaIndex).toArray, forDevice.map(_.instance.instanceNumber).toArray,
                            Array.tabulate(k)(first + _))
        val (sets, ws, tg) = (keyset.map(x => (if (x._2) 1 else 0).toByte).toArray,
                              forDevice.flatMap(c => watermarks(c.dependencies)).toArray, Array.fill(k)(bit(index)))
        Native.check(if (engine.singleKeys(ks)) Native.epxHandleCommit(engine.handle, k, n, ls, ns, ts, engine.singleKey(ks), sets, ws, endsIn, tg)
                     else Native.epxHandleCommitMk(engine.handle, k, n, ls, ns, ts, engine.keyOffsets(ks), engine.keyList(ks), sets, ws,
                                                   endsIn, tg), logger)
        for ((c, i) <- forDevice.zipWithIndex) endsOf(c) = endsIn(i)
      }
      for (c <- commits) {
        endsOf.get(c).foreach(end => engine.depsOf((c.instance.replicaIndex, c.instance.instanceNumber)) = (watermarks(c.dependencies), end))
        learnCommit(c.instance, c.commandOrNoop, c.dependencies)
      }
      commits.clear()
      executeGraph()
    }
    // ---- PreAccepts from replicas outside (a leader's re-sent PreAccept, a recovering replica's): Replica.handlePreAccept
    // in full (:1159-1289) at THIS replica; Nack / PreAcceptOk / Commit back to the sender
    if (preAccepts.nonEmpty) {
      val k = preAccepts.size
      val ps = preAccepts.map(_._2)
      val keyset = ps.map(p => engine.classify(p.commandOrNoop)); val ks = keyset.map(_._1)
      val first = engine.triples.size; ps.foreach(p => engine.triples += p.commandOrNoop)
      val depsIn = ps.flatMap(p => watermarks(p.dependencies)).toArray
      val endsIn = ps.map(p => { val v = p.dependencies.intPrefixSet(p.instance.replicaIndex).value; if (v.isEmpty) 0 else v.max + 1 }).toArray
      val replies = new Array[Byte](4 * k); val nb = new Array[Int](k); val rd = new Array[Int](k * n * n); val ret = new Array[Int](2 * k * n)
      val (ls, ns, bo, br) = (ps.map(_.instance.replicaIndex).toArray, ps.map(_.instance.instanceNumber).toArray,
                              ps.map(_.ballot.ordering).toArray, ps.map(_.ballot.replicaIndex).toArray)
      val sets = keyset.map(x => (if (x._2) 1 else 0).toByte).toArray
      Native.check(if (engine.singleKeys(ks))
                     Native.epxHandlePreaccept(engine.handle, k, n, ls, ns, bo, br, engine.singleKey(ks), sets, Array.tabulate(k)(first + _),
                                               depsIn, endsIn, Array.fill(k)(bit(index)), replies, nb, rd, ret)
                   else
                     Native.epxHandlePreacceptMk(engine.handle, k, n, ls, ns, bo, br, engine.keyOffsets(ks), engine.keyList(ks), sets,
                                                 Array.tabulate(k)(first + _), depsIn, endsIn, Array.fill(k)(bit(index)), replies, nb,
                                                 rd, ret), logger)
      for (((src, p), i) <- preAccepts.zipWithIndex) {
        val back = chan[Replica[Transport]](src, Replica.serializer)
        val mine = (replies(i) & bit(index)) != 0 || (replies(k + i) & bit(index)) != 0        // processed, or answered again
        if ((replies(2 * k + i) & bit(index)) != 0)                                             // :1176-1186 Nack(instance, largestBallot)
          back.send(ReplicaInbound().withNack(Nack(p.instance, Ballot(nb(i) >> 3, nb(i) & 7))))
        else if (mine) {
          val w = rd.slice((i * n + index) * n, (i * n + index + 1) * n)
          back.send(ReplicaInbound().withPreAcceptOk(PreAcceptOk(p.instance, p.ballot, index, 0,
            prefixSet(w, p.instance.replicaIndex, ret(i * n + index), p.instance.instanceNumber))))
        } else if ((replies(3 * k + i) & bit(index)) != 0)                                      // :1228-1238 the Commit back
          engine.depsOf.get((p.instance.replicaIndex, p.instance.instanceNumber)).foreach { case (w, end) =>
            back.send(ReplicaInbound().withCommit(Commit(p.instance, engine.triples(ret(k * n + i * n + index)), 0,
                                                         prefixSet(w, p.instance.replicaIndex, end, p.instance.instanceNumber))))
          }
      }
      preAccepts.clear()
    }
    // ---- Accepts (:1421-1511) and Prepares (:1632-1757) from replicas outside, at THIS replica
    if (accepts.nonEmpty) {
      val k = accepts.size; val as = accepts.map(_._2)
      val keyset = as.map(a => engine.classify(a.commandOrNoop)); val ks = keyset.map(_._1)
      val first = engine.triples.size; as.foreach(a => engine.triples += a.commandOrNoop)
      for ((a, i) <- as.zipWithIndex) {   // the device keeps an accepted triple by its id: its dependencies stay here
        val v = a.dependencies.intPrefixSet(a.instance.replicaIndex).value
        engine.tripleDeps(first + i) = (watermarks(a.dependencies), if (v.isEmpty) 0 else v.max + 1)
      }
      val replies = new Array[Byte](4 * k); val nb = new Array[Int](k)
      val (ls, ns, bo, br, ts) = (as.map(_.instance.replicaIndex).toArray, as.map(_.instance.instanceNumber).toArray,
                                  as.map(_.ballot.ordering).toArray, as.map(_.ballot.replicaIndex).toArray, Array.tabulate(k)(first + _))
      val sets = keyset.map(x => (if (x._2) 1 else 0).toByte).toArray
      Native.check(if (engine.singleKeys(ks))
                     Native.epxAccept(engine.handle, k, ls, ns, bo, br, ts, engine.singleKey(ks), sets, Array.fill(k)(bit(index)), replies, nb)
                   else
                     Native.epxAcceptMk(engine.handle, k, ls, ns, bo, br, ts, engine.keyOffsets(ks), engine.keyList(ks), sets,
                                        Array.fill(k)(bit(index)), replies, nb), logger)
      for (((src, a), i) <- accepts.zipWithIndex) {
        val back = chan[Replica[Transport]](src, Replica.serializer)
        if ((replies(i) & bit(index)) != 0) back.send(ReplicaInbound().withAcceptOk(AcceptOk(a.instance, a.ballot, index)))
        else if ((replies(k + i) & bit(index)) != 0) back.send(ReplicaInbound().withNack(Nack(a.instance, Ballot(nb(i) >> 3, nb(i) & 7))))
      }
      accepts.clear()
    }
    if (prepares.nonEmpty) {
      val k = prepares.size; val ps = prepares.map(_._2)
      val replies = new Array[Byte](3 * k); val nb = new Array[Int](k); val ok = new Array[Int](3 * k * n)
      Native.check(Native.epxPrepare(engine.handle, k, n, ps.map(_.instance.replicaIndex).toArray, ps.map(_.instance.instanceNumber).toArray,
                                     ps.map(_.ballot.ordering).toArray, ps.map(_.ballot.replicaIndex).toArray, Array.fill(k)(bit(index)),
                                     replies, nb, ok), logger)
      for (((src, p), i) <- prepares.zipWithIndex) {
        val back = chan[Replica[Transport]](src, Replica.serializer)
        val L = p.instance.replicaIndex; val x = p.instance.instanceNumber
        if ((replies(k + i) & bit(index)) != 0) back.send(ReplicaInbound().withNack(Nack(p.instance, Ballot(nb(i) >> 3, nb(i) & 7))))
        else if ((replies(2 * k + i) & bit(index)) != 0) {
          // :1746-1756 a CommittedEntry: "No need to run the protocol" -- the Commit goes back
          val entry = new Array[Int](6 + n)
          Native.check(Native.epxReadCmdlog(engine.handle, n, index, L, x, entry), logger)
          engine.depsOf.get((L, x)).foreach { case (w, end) =>
            back.send(ReplicaInbound().withCommit(Commit(p.instance, engine.triples(entry(3)), 0, prefixSet(w, L, end, x))))
          }
        } else if ((replies(i) & bit(index)) != 0) {
          val status = ok(i * n + index); val vote = ok(k * n + i * n + index); val triple = ok(2 * k * n + i * n + index)
          // the entry's triple: its dependencies are in the command log (what THIS replica answered the PreAccept with), or
          // -- an entry an Accept wrote names its triple by id -- with the engine (tripleDeps)
          val seen = status != 0 && triple >= 0
          val deps: Option[InstancePrefixSetProto] =
            if (!seen) None
            else {
              val entry = new Array[Int](6 + n)
              Native.check(Native.epxReadCmdlog(engine.handle, n, index, L, x, entry), logger)
              val (w, end) = if (entry(5) >= 0) (entry.slice(5, 5 + n), entry(5 + n))
                             else engine.tripleDeps.getOrElse(triple, engine.depsOf.getOrElse((L, x), (Array.fill(n)(0), 0)))
              Some(prefixSet(w, L, end, x))
            }
          back.send(ReplicaInbound().withPrepareOk(PrepareOk(
            ballot = p.ballot, instance = p.instance, replicaIndex = index,
            voteBallot = if (vote < 0) Replica.nullBallot else Ballot(vote >> 3, vote & 7),       // (-1, -1), Replica.scala:256
            status = status match { case 0 | 1 => CommandStatus.NotSeen; case 2 => CommandStatus.PreAccepted; case _ => CommandStatus.Accepted },
            commandOrNoop = if (seen) Some(engine.triples(triple)) else None,
            sequenceNumber = if (seen) Some(0) else None,                                          // :1711-1737
            dependencies = deps)))
        }
      }
      prepares.clear()
    }
    // ---- replies to the instances this replica leads (remotePeers), after the burst's PreAccepts / Accepts / Prepares /
    // Commits have moved the command log: a reply for an instance that was taken away finds its leader state gone
    if (leaderInbox.nonEmpty) flushLeaderReplies()
    queued = 0
  }

  // replicas of this process: the addresses a GpuEPaxosReplica was created for (set by the main that creates them)
  var hosted: Transport#Address => Boolean = _ => true
}
