"""epaxos_reply_cases.py -- TEST INFRASTRUCTURE ONLY: the records of an EPaxos replica tick (what fpx_epx_replica_inbox
answers, include/fpx.h) and the replies they must become (include/fpx_wire.h, fpx_wire_epx_encode_replica_replies): a
case set on every varint boundary, the reply of a record written a second time in Python with the assembler of
epaxos_wire_cases.py, and the same reply from the yardstick, fpx_wire_epaxos_encode_replica_inbound, one message at a time."""
import numpy as np

from tests.epaxos_wire_cases import accept_ok, deps_body, i32, ld, nack, pair, pre_accept_ok, prefix_set

NONE, ENCODED, DEFERRED = 0, 1, 2
IDS_MAX = 64                    # FPX_WIRE_EPX_FOLD_MAX
I32_MAX = (1 << 31) - 1
# both sides of every varint boundary of a non-negative int32
BOUNDS = (0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, I32_MAX)
ORDERINGS = (0, 127, 128, (1 << 27) - 1)
FIELDS = ("to", "leader", "number", "ballot_ordering", "ballot_replica", "outcome", "out_ballot", "out_status", "out_deps",
          "out_values_end")


def rec(n, to, leader, number, ballot, outcome, out_ballot=-1, out_status=-1, deps=None, values_end=0):
    """one record, as a tuple in FIELDS order; deps: n watermarks (default zeros)"""
    deps = [0] * n if deps is None else list(deps)
    assert len(deps) == n
    return (to, leader, number, ballot[0], ballot[1], outcome, out_ballot, out_status, tuple(deps), values_end)


def arrays(n, records):
    """the records as the ten arrays the encoders take (a dict by FIELDS)"""
    cols = list(zip(*records)) if records else [()] * len(FIELDS)
    out = {k: np.array(c, dtype=np.int64).astype(np.int32) for k, c in zip(FIELDS, cols)}
    out["out_deps"] = out["out_deps"].reshape(len(records), n)
    return out


def own_ids(r):
    """the explicit ids of the own-leader column: number + 1 .. values_end - 1 when values_end > 0"""
    number, end = r[2], r[9]
    return list(range(number + 1, end)) if end > 0 else []


def prepare_ok(ballot, inst, replica, vote_ballot, status):
    """PrepareOk { ballot = 1; instance = 2; replica_index = 3; vote_ballot = 4; status = 5 } without its optional fields"""
    return ld(8, pair(1, *ballot) + pair(2, *inst) + i32(3, replica) + pair(4, *vote_ballot) + i32(5, status))


def plan(n, r):
    """the reply kind of a record (the table of include/fpx_wire.h), None for an unknown outcome"""
    outcome, status, deps = r[5], r[7], r[8]
    if outcome in (0, 5):
        return NONE
    if outcome in (1, 2):
        return DEFERRED if deps[0] < 0 or len(own_ids(r)) > IDS_MAX else ENCODED
    if outcome in (3, 4, 7):
        return ENCODED
    if outcome == 6:
        return ENCODED if status == 0 else DEFERRED
    if outcome == 8:
        return DEFERRED
    return None


def py_reply(n, r):
    """(kind, bytes) of a record, from the assembler"""
    to, leader, number, bo, br, outcome, ob, status, deps, end = r
    kind = plan(n, r)
    if kind != ENCODED:
        return kind, b""
    inst, ballot = (leader, number), (bo, br)
    if outcome in (1, 2):
        sets = [prefix_set(deps[l], own_ids(r) if l == leader else ()) for l in range(n)]
        return kind, pre_accept_ok(inst, ballot, to, 0, deps_body(sets))
    if outcome in (3, 4):
        return kind, accept_ok(inst, ballot, to)
    if outcome == 7:
        return kind, nack(inst, (ob >> 3, ob & 7))
    return kind, prepare_ok(ballot, inst, to, (-1, -1) if ob < 0 else (ob >> 3, ob & 7), 0)


def yardstick_reply(wire, n, r):
    """the same from fpx_wire_epaxos_encode_replica_inbound, called once for this message"""
    to, leader, number, bo, br, outcome, ob, status, deps, end = r
    if plan(n, r) != ENCODED:
        return b""
    inst, ballot = (leader, number), (bo, br)
    if outcome in (1, 2):
        return wire.epaxos_encode(wire.EPX_PRE_ACCEPT_OK, inst, ballot, replica_index=to, sequence_number=0, deps=list(deps),
                                  values=[(leader, v) for v in own_ids(r)])
    if outcome in (3, 4):
        return wire.epaxos_encode(wire.EPX_ACCEPT_OK, inst, ballot, replica_index=to)
    if outcome == 7:
        return wire.epaxos_encode(wire.EPX_NACK, inst, (ob >> 3, ob & 7))
    return wire.epaxos_encode(wire.EPX_PREPARE_OK, inst, ballot, replica_index=to,
                              vote_ballot=(-1, -1) if ob < 0 else (ob >> 3, ob & 7), status=0)


def id_run(n, leader, count, first_id, outcome=1, ordering=5):
    """a PreAcceptOk record whose own column carries `count` explicit ids first_id .. (count 0: values_end 0)"""
    number = first_id - 1
    deps = [(7 * l + 3) % 200 for l in range(n)]
    deps[leader] = number                       # ids need the own-leader watermark at the instance number
    return rec(n, (leader + 1) % n, leader, number, (ordering, leader), outcome, deps=deps,
               values_end=first_id + count if count else 0)


def worst_case(n):
    """the longest reply there is at n: 64 five-byte ids, every number and watermark at five bytes, the widest ordering"""
    number = I32_MAX - 1 - IDS_MAX
    deps = [I32_MAX] * n
    deps[n - 1] = number
    return rec(n, n - 1, n - 1, number, (ORDERINGS[-1], n - 1), 1, deps=deps, values_end=I32_MAX)


def case_records(n):
    """the case set of the issue at n replicas, as a list of records"""
    out = []
    bal = (9, 1)
    # every outcome
    for outcome in range(9):
        out.append(rec(n, 1, 2 % n, 40 + outcome, bal, outcome, out_ballot=(12 << 3) | 2 if outcome in (6, 7) else -1,
                       out_status=0 if outcome == 6 else -1, deps=[5 + l for l in range(n)]))
    # instance numbers and watermarks on both sides of every varint boundary, in every reply
    for j, b in enumerate(BOUNDS):
        leader, to = j % n, (j + 1) % n
        deps = [BOUNDS[(j + l) % len(BOUNDS)] for l in range(n)]
        deps[leader] = min(deps[leader], b)
        out.append(rec(n, to, leader, b, bal, 1 + j % 2, deps=deps))
        out.append(rec(n, to, leader, b, bal, 3 + j % 2))
        out.append(rec(n, to, leader, b, bal, 7, out_ballot=(b >> 4 << 3) | to))
        out.append(rec(n, to, leader, b, bal, 6, out_ballot=-1 if j % 2 else (j << 3) | leader, out_status=0))
    # the ballot's ordering, the message's and the reply's own
    for j, o in enumerate(ORDERINGS):
        leader, to = (j + 1) % n, j % n
        out.append(rec(n, to, leader, 77, (o, leader), 1, deps=[3] * n))
        out.append(rec(n, to, leader, 77, (o, leader), 3))
        out.append(rec(n, to, leader, 77, (o, leader), 7, out_ballot=(o << 3) | (n - 1)))
        out.append(rec(n, to, leader, 77, (o, leader), 6, out_ballot=(o << 3) | to, out_status=0))
        out.append(rec(n, to, leader, 77, (o, leader), 6, out_ballot=-1, out_status=0))
    # explicit-id counts, the runs straddling the varint boundaries (65: deferred)
    for j, count in enumerate((0, 1, 63, 64, 65)):
        for edge in (128, 16384, 1 << 21, 1 << 28):
            out.append(id_run(n, j % n, count, max(edge - count // 2, 1), outcome=1 + j % 2))
        out.append(id_run(n, j % n, count, 1))                              # number 0
        out.append(id_run(n, j % n, count, I32_MAX - count))                # the last id is 2^31 - 2
    leader = 1
    out.append(rec(n, 0, leader, 300, bal, 1, deps=[2, 300] + [2] * (n - 2), values_end=301))   # values_end > 0, no id
    # a triple stored by id: the host has its dependencies
    out.append(rec(n, 0, leader, 9, bal, 1, deps=[-1] * n))
    out.append(rec(n, 0, leader, 9, bal, 2, deps=[-1] + [4] * (n - 1), values_end=12))
    # PrepareOk by status: NotSeen is encoded, the two that carry a command are the caller's
    for status in (0, 2, 3):
        out.append(rec(n, 2, 0, 31, bal, 6, out_ballot=(3 << 3) | 1, out_status=status, deps=[1] * n))
    out.append(worst_case(n))
    return out


def short_reply(n, j):
    """a record whose reply is one of the short ones (AcceptOk, Nack, PreAcceptOk without ids, PrepareOk), by j"""
    leader, to = j % n, (j + 2) % n
    what = j % 4
    if what == 0:
        return rec(n, to, leader, 100 + j, (j, leader), 1, deps=[j + l for l in range(n)])
    if what == 1:
        return rec(n, to, leader, 100 + j, (j, leader), 3)
    if what == 2:
        return rec(n, to, leader, 100 + j, (j, leader), 7, out_ballot=((j + 1) << 3) | to)
    return rec(n, to, leader, 100 + j, (j, leader), 6, out_ballot=-1, out_status=0)


def wave_records(n):
    """wavefronts of 64 records each: one whose records all send nothing, one that is all deferred, one that holds a single
    64-id PreAcceptOk among short replies, one of short replies alone"""
    none = [rec(n, 0, 1, j, (1, 1), (0, 5)[j % 2]) for j in range(64)]
    deferred = [(rec(n, 0, 1, j, (1, 1), 8), rec(n, 0, 1, j, (1, 1), 6, out_ballot=9, out_status=2),
                 rec(n, 0, 1, j, (1, 1), 1, deps=[-1] * n))[j % 3] for j in range(64)]
    long_one = [short_reply(n, j) for j in range(64)]
    long_one[37] = id_run(n, 1, 64, 16384 - 32)
    shorts = [short_reply(n, j) for j in range(64)]
    return none + deferred + long_one + shorts


def burst(n, m, shift=0):
    """m records: the case set and the wavefronts, repeated and rotated by `shift`"""
    base = wave_records(n) + case_records(n)
    base = base[shift % len(base):] + base[:shift % len(base)]
    return [base[j % len(base)] for j in range(m)]


def expected(n, records):
    """(replies, kinds, offsets, totals) from the Python writer"""
    got = [py_reply(n, r) for r in records]
    replies, kinds = [g[1] for g in got], [g[0] for g in got]
    offsets = np.zeros(len(records) + 1, np.int64)
    np.cumsum([len(b) for b in replies], out=offsets[1:])
    totals = np.array([kinds.count(ENCODED), int(offsets[-1]), kinds.count(DEFERRED), -1], np.int64)
    return replies, np.array(kinds, np.uint8), offsets, totals
