"""Leader.handlePhase1b of the reference, restated one message at a time (multipaxos/Leader.scala:306-329, 504-577;
mencius/Leader.scala:359-385, 582-659): a dict of Phase1bs per acceptor group, `find` per slot per message, `maxBy` on
the vote round.  This is what fpx_leader_phase1b_msgs must compute for a burst; it is written from the Scala and shares
no code with the library.

Where the Scala leaves something open the contract of include/fpx.h is stated here too: ties of maxBy go to the lowest
acceptor bit, the checks that make a burst FPX_EINVAL, and what a logger.check that fires turns into."""
from dataclasses import dataclass, field

OK, EINVAL, ECAPACITY, EFATAL_PROTOCOL = 0, 1, 5, 9
NOOP = -1
PHASE1B = 9          # FPX_WIRE_PHASE1B
MAX_ROUND = 2 ** 30 - 2
GRID = 2             # FPX_Q_GRID


@dataclass
class Msg:
    round: int
    group: int
    acceptor: int
    info: list = field(default_factory=list)   # [(slot, vote_round, value_id)], as the acceptor sent them
    kind: int = PHASE1B


@dataclass
class Geometry:
    num_groups: int = 1
    num_leader_groups: int = 1
    f: int = 1
    total: int = 3               # acceptors per group (replicas_total)
    quorum_kind: int = 0
    grid_rows: int = 0
    grid_cols: int = 0


@dataclass
class Result:
    status: int = OK
    err_index: int = -1
    complete: int = None         # None: nothing was written
    decided_at: int = None
    max_slot: int = None
    next_slot: int = None
    count: int = None
    out_slot: list = None
    safe_round: list = None
    safe_value: list = None
    held: set = None             # {(group, bit)}: the acceptors used


def next_classic_round(n, leader, rnd):
    """RoundSystem.ClassicRoundRobin(n).nextClassicRound (roundsystem/RoundSystem.scala:66-81)"""
    if rnd < 0:
        return leader
    m = n * (rnd // n)
    return m + leader if m + leader > rnd else m + n + leader


def is_read_quorum(geo, bits):
    """the context's read-quorum predicate over a set of bits (Grid.scala:36-41: some row wholly held)"""
    if geo.quorum_kind == GRID:
        return any(all(r * geo.grid_cols + c in bits for c in range(geo.grid_cols)) for r in range(geo.grid_rows))
    if geo.quorum_kind == 0:
        return len(bits) >= geo.total - geo.f
    raise NotImplementedError


def bit_of(m, grid_cols):
    return m.group * grid_cols + m.acceptor if grid_cols > 0 else m.acceptor


def header_ok(geo, m, grid_cols):
    if m.group < 0 or m.acceptor < 0:
        return False
    if grid_cols > 0:
        return m.acceptor < grid_cols and bit_of(m, grid_cols) < geo.total
    return m.group < geo.num_groups and m.acceptor < geo.total


def info_ok(info):
    prev = -1
    for slot, vr, _ in info:
        if slot < 0 or slot <= prev or not 0 <= vr <= MAX_ROUND:
            return False
        prev = slot
    return True


_first_of = {}


def find(m, slot):
    """m.info.find(_.slot == slot): the FIRST record of the slot (an index per message, built once: the streams have
    thousands of slots)"""
    index = _first_of.get(id(m))
    if index is None or index[0] is not m:
        by_slot = {}
        for rec in reversed(m.info):
            by_slot[rec[0]] = rec
        index = _first_of[id(m)] = (m, by_slot)
    return index[1].get(slot)


def handle_burst(geo, round_, watermark, msgs, leader_group=0, recover_slot=-1, grid_cols=0, all_rows=False, cap=None,
                 offsets_bad_at=None):
    """offsets_bad_at: the lowest message index whose offsets do not ascend (the model's messages carry lists, so the
    caller says where the flat arrays it built from them are broken)."""
    res = Result()
    L = geo.num_leader_groups
    # ---- the headers of the whole burst, before anything else
    bad = [i for i, m in enumerate(msgs) if m.kind == PHASE1B and not header_ok(geo, m, grid_cols)]
    if offsets_bad_at is not None:
        bad.append(offsets_bad_at)
    if bad:
        res.status, res.err_index = EINVAL, min(bad)
        return res
    # ---- message by message
    ngroups = (geo.total + grid_cols - 1) // grid_cols if grid_cols > 0 else geo.num_groups
    phase1bs = [dict() for _ in range(ngroups)]          # phase1.phase1bs: group -> acceptor -> Phase1b
    held = set()                                         # phase1.phase1bAcceptors
    index_of = {}
    k = None
    for i, m in enumerate(msgs):
        if m.kind != PHASE1B:
            continue
        if m.round != round_:                            # :517-526
            if m.round > round_ and res.status == OK:    # logger.checkLt(phase1b.round, round)
                res.status, res.err_index = EFATAL_PROTOCOL, i
            continue
        phase1bs[m.group][m.acceptor] = m
        index_of[(m.group, m.acceptor)] = i
        if grid_cols > 0:
            held.add(bit_of(m, grid_cols))
            if not is_read_quorum(geo, held):
                continue
        elif any(len(g) < geo.f + 1 for g in phase1bs):
            continue
        k = i
        break                                            # the leader is in Phase 2: the rest is ignored
    if k is None:
        res.complete, res.decided_at = 0, -1
        return res
    used = [m for g in phase1bs for m in g.values()]
    badrec = [index_of[(m.group, m.acceptor)] for m in used if not info_ok(m.info)]
    if badrec:
        return Result(status=EINVAL, err_index=min(badrec))
    max_slot = max([max((s for s, _, _ in m.info), default=-1) for m in used] + [recover_slot])
    if max_slot != -1 and max_slot % L != leader_group:  # logger.check(maxSlot == -1 || slotSystem.leader(maxSlot) == groupIndex)
        return Result(status=EFATAL_PROTOCOL, err_index=res.err_index if res.status != OK else -1)
    res.complete, res.decided_at, res.max_slot = 1, k, max_slot
    res.out_slot, res.safe_round, res.safe_value = [], [], []
    for slot in range(next_classic_round(L, leader_group, watermark - 1), max_slot + 1, L):
        if grid_cols > 0:
            group = used if all_rows else list(phase1bs[slot % ngroups].values())            # Leader.scala:552
        else:
            group = list(phase1bs[(slot // L) % geo.num_groups].values())
        # safeValue: phase1bs.flatMap(_.info.find(_.slot == slot)), maxBy(_.voteRound); ties: the lowest bit
        best = None
        for m in sorted(group, key=lambda m: bit_of(m, grid_cols)):
            hit = find(m, slot)
            if hit is not None and (best is None or hit[1] > best[1]):
                best = hit
        res.out_slot.append(slot)
        res.safe_round.append(-1 if best is None else best[1])
        res.safe_value.append(NOOP if best is None else best[2])
    res.count = len(res.out_slot)
    res.next_slot = next_classic_round(L, leader_group, max_slot)
    res.held = {(0 if grid_cols > 0 else leader_group * geo.num_groups + m.group, bit_of(m, grid_cols)) for m in used}
    if cap is not None and res.count > cap:
        if res.status == OK:
            res.status = ECAPACITY
        res.out_slot, res.safe_round, res.safe_value = res.out_slot[:cap], res.safe_round[:cap], res.safe_value[:cap]
    return res


def flatten(msgs):
    """the arrays the entry points take: kind, msg_round, group_index, acceptor_index, offsets, info_slot,
    info_vote_round, info_value_id"""
    import numpy as np

    off = np.zeros(len(msgs) + 1, np.int64)
    for i, m in enumerate(msgs):
        off[i + 1] = off[i] + len(m.info)
    rec = [r for m in msgs for r in m.info]
    col = lambda j: np.array([r[j] for r in rec], np.int32)
    return dict(kind=np.array([m.kind for m in msgs], np.int32), msg_round=np.array([m.round for m in msgs], np.int32),
                group_index=np.array([m.group for m in msgs], np.int32),
                acceptor_index=np.array([m.acceptor for m in msgs], np.int32), offsets=off,
                info_slot=col(0), info_vote_round=col(1), info_value_id=col(2))
