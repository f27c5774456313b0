"""epaxos_cmd_reply_cases.py -- TEST INFRASTRUCTURE ONLY: command stores as plain arrays (what fpx_epx_cmds_* keeps on the
device, include/fpx.h) and the records of a replica tick whose replies carry a stored command -- the Commit sent back and the
PrepareOk of a PreAccepted / Accepted instance (include/fpx_wire.h, "with the command store").  One generator for the CPU and
the GPU tests: the records (epaxos_reply_cases.py's tuples with the triple id appended), the reply of a record written a
second time in Python, and the same reply from the yardstick, fpx_wire_epaxos_encode_replica_inbound."""
import numpy as np

from tests import epaxos_reply_cases as RC
from tests.epaxos_wire_cases import deps_body, i32, ld, pair, prefix_set, varint

NONE, ENCODED, DEFERRED = RC.NONE, RC.ENCODED, RC.DEFERRED
CMD_MAX_LEN = 1 << 16                       # FPX_EPX_CMD_MAX_LEN
CMD_LENS = (0, 1, 2, 127, 128, CMD_MAX_LEN)
NOOP = bytes([0x12, 0x00])                  # CommandOrNoop { noop = 2: {} }
FIELDS = RC.FIELDS + ("out_triple",)


def command(length, salt=0):
    """a CommandOrNoop { command = 1 } of exactly `length` bytes whose body differs by position and by salt (the store and
    the encoder take it as opaque bytes; the decoder of the round trip wants the oneof).  Below two bytes there is no such
    message: those are bytes the store keeps verbatim all the same"""
    fill = lambda k: bytes((17 * salt + 31 * j + (j >> 8)) & 0xff for j in range(k))
    for head in (2, 3, 4):
        body = length - head
        if body >= 0 and 1 + len(varint(body)) == head:
            return b"\x0a" + varint(body) + fill(body)
    assert length < 2
    return fill(length)


class Store:
    """triple id -> bytes, laid out as the device lays it out: the arena in order of insertion, offsets -1 = no bytes"""

    def __init__(self, max_triples):
        self.max_triples = max_triples
        self.off = np.full(max_triples, -1, np.int64)
        self.len = np.zeros(max_triples, np.int32)
        self.arena = bytearray()

    def put(self, triple, data):
        assert 0 <= triple < self.max_triples and self.off[triple] < 0
        self.off[triple], self.len[triple] = len(self.arena), len(data)
        self.arena += data
        return triple

    def get(self, triple):
        if not 0 <= triple < self.max_triples or self.off[triple] < 0:
            return None
        o = int(self.off[triple])
        return bytes(self.arena[o:o + int(self.len[triple])])

    def arrays(self):
        """(cmd_off, cmd_len, arena): the arena a block of exactly the bytes used"""
        return self.off, self.len, np.frombuffer(bytes(self.arena), np.uint8)


def rec(n, to, leader, number, ballot, outcome, triple, out_ballot=-1, out_status=-1, deps=None, values_end=0):
    return RC.rec(n, to, leader, number, ballot, outcome, out_ballot, out_status, deps, values_end) + (triple,)


def arrays(n, records):
    """the records as the ten arrays of the encoders and out_triple (a dict by FIELDS)"""
    out = RC.arrays(n, [r[:10] for r in records])
    out["out_triple"] = np.array([r[10] for r in records], np.int64).astype(np.int32)
    return out


def plan(n, r, store):
    """the reply kind of a record with a store (None: without one)"""
    outcome, status, deps, triple = r[5], r[7], r[8], r[10]
    carries = outcome == 8 or (outcome == 6 and status in (2, 3))
    if not carries or store is None:
        return RC.plan(n, r[:10])
    if store.get(triple) is None or deps[0] < 0 or len(RC.own_ids(r)) > RC.IDS_MAX:
        return DEFERRED
    return ENCODED


def py_reply(n, r, store):
    """(kind, bytes) of a record, from the assembler"""
    kind = plan(n, r, store)
    to, leader, number, bo, br, outcome, ob, status, deps, end, triple = r
    carries = outcome == 8 or (outcome == 6 and status in (2, 3))
    if not carries or store is None:
        return RC.py_reply(n, r[:10])
    if kind != ENCODED:
        return kind, b""
    cmd = store.get(triple)
    sets = [prefix_set(deps[l], RC.own_ids(r) if l == leader else ()) for l in range(n)]
    d = deps_body(sets)
    if outcome == 8:
        return kind, ld(6, pair(1, leader, number) + ld(2, cmd) + i32(3, 0) + ld(4, d))
    vote = (-1, -1) if ob < 0 else (ob >> 3, ob & 7)
    return kind, ld(8, pair(1, bo, br) + pair(2, leader, number) + i32(3, to) + pair(4, *vote) + i32(5, status - 1) + ld(6, cmd) +
                    i32(7, 0) + ld(8, d))


def yardstick_reply(wire, n, r, store):
    """the same from fpx_wire_epaxos_encode_replica_inbound, called once for this message"""
    to, leader, number, bo, br, outcome, ob, status, deps, end, triple = r
    if plan(n, r, store) != ENCODED:
        return b""
    carries = outcome == 8 or (outcome == 6 and status in (2, 3))
    if not carries or store is None:
        return RC.yardstick_reply(wire, n, r[:10])
    cmd = store.get(triple)
    if not cmd:
        # an EMPTY CommandOrNoop (no oneof member) is nothing the yardstick sends or the decoder takes (wire._val); the
        # store keeps bytes verbatim all the same, so length 0 is held against the Python writer alone
        return None
    values = [(leader, v) for v in RC.own_ids(r)]
    if outcome == 8:
        return wire.epaxos_encode(wire.EPX_COMMIT, (leader, number), sequence_number=0, command=cmd, deps=list(deps), values=values)
    return wire.epaxos_encode(wire.EPX_PREPARE_OK, (leader, number), (bo, br), replica_index=to, sequence_number=0,
                              vote_ballot=(-1, -1) if ob < 0 else (ob >> 3, ob & 7), status=status - 1, command=cmd,
                              deps=list(deps), values=values)


def cmd_reply(n, j, triple, ids=0, out_ballot=None):
    """a record whose reply carries triple's command, by j: a Commit back, a PrepareOk PreAccepted, a PrepareOk Accepted"""
    leader, to = j % n, (j + 1) % n
    number = 50 + j
    deps = [(5 * l + j) % 90 for l in range(n)]
    deps[leader] = min(deps[leader], number)
    if ids:
        deps[leader] = number
    end = number + 1 + ids if ids else 0
    what = j % 3
    if what == 0:
        return rec(n, to, leader, number, (j % 100, leader), 8, triple, deps=deps, values_end=end)
    ob = ((j % 50) << 3) | to if out_ballot is None else out_ballot
    return rec(n, to, leader, number, (j % 100, leader), 6, triple, out_ballot=ob, out_status=1 + what, deps=deps, values_end=end)


def worst_case(n, triple):
    """the longest reply that carries triple's command: a PrepareOk with nullBallot, 64 five-byte ids, every number and
    watermark at five bytes, the widest ordering"""
    number = RC.I32_MAX - 1 - RC.IDS_MAX
    deps = [RC.I32_MAX] * n
    deps[n - 1] = number
    return rec(n, n - 1, n - 1, number, (RC.ORDERINGS[-1], n - 1), 6, triple, out_ballot=-1, out_status=3, deps=deps,
               values_end=RC.I32_MAX)


def case_store(max_triples=64):
    """a store with a Noop, commands of every length of CMD_LENS, and ids without bytes; (store, {length: id}, noop id)"""
    s = Store(max_triples)
    noop = s.put(3, NOOP)
    by_len = {}
    for k, length in enumerate(CMD_LENS):
        by_len[length] = s.put(5 + 2 * k, command(length, salt=k))     # (the even ids in between have no bytes)
    return s, by_len, noop


def case_records(n, by_len, noop, max_triples):
    """the case set of the issue at n replicas"""
    out = []
    j = 0
    for length in CMD_LENS:
        for what in range(3):                                          # Commit back, PreAccepted, Accepted
            out.append(cmd_reply(n, 3 * j + what, by_len[length]))
        j += 1
    for what in range(3):
        out.append(cmd_reply(n, 30 + what, noop))
    # explicit ids in the own column: 1 and 64 are encoded, 65 is deferred
    for ids in (1, 64, 65):
        for what in range(3):
            out.append(cmd_reply(n, 60 + 3 * ids + what, by_len[127], ids=ids))
    # nullBallot in a PrepareOk with a command
    out.append(cmd_reply(n, 91, by_len[2], out_ballot=-1))
    out.append(cmd_reply(n, 92, by_len[128], out_ballot=-1))
    # every way back to deferred: an id out of range (both sides), an id without bytes, dependencies by id
    for triple in (-1, max_triples, max_triples + 7, 4, 0):
        for what in range(3):
            out.append(cmd_reply(n, 120 + what, triple))
    for what in range(3):
        r = cmd_reply(n, 150 + what, by_len[1])
        out.append(r[:8] + ((-1,) + r[8][1:],) + r[9:])
    # the other PrepareOk statuses are what they were: 0 encoded without a command, 1 deferred
    out.append(rec(n, 1, 0, 31, (9, 1), 6, by_len[1], out_ballot=(3 << 3) | 1, out_status=0, deps=[1] * n))
    out.append(rec(n, 1, 0, 31, (9, 1), 6, by_len[1], out_ballot=(3 << 3) | 1, out_status=1, deps=[1] * n))
    out.append(worst_case(n, by_len[CMD_MAX_LEN]))
    out.append(worst_case(n, by_len[0]))
    return out


def short(n, j):
    return RC.short_reply(n, j) + (-1,)


def wave_records(n, by_len):
    """two wavefronts of 64 records: one of short replies alone (the span form), one of short replies with a single command
    reply (the direct form)"""
    shorts = [short(n, j) for j in range(64)]
    one = [short(n, j) for j in range(64)]
    one[21] = cmd_reply(n, 7, by_len[128])
    return shorts + one


def burst(n, m, by_len, noop, max_triples, shift=0, only_cmds=False, big=True):
    """m records: command replies alone, or the waves, the case set and epaxos_reply_cases.py's short cases mixed; big False
    leaves the FPX_EPX_CMD_MAX_LEN commands out (a burst of many records stays small)"""
    cases = case_records(n, by_len, noop, max_triples)
    if not big:
        cases = [r for r in cases if r[10] != by_len[CMD_MAX_LEN]]
    if only_cmds:
        base = [r for r in cases if r[5] == 8 or (r[5] == 6 and r[7] in (2, 3))]
    else:
        base = wave_records(n, by_len) + cases + [r + (-1,) for r in RC.case_records(n)]
    base = base[shift % len(base):] + base[:shift % len(base)]
    return [base[j % len(base)] for j in range(m)]


def expected(n, records, store):
    """(replies, kinds, offsets, totals) from the Python writer"""
    got = [py_reply(n, r, store) for r in records]
    replies, kinds = [g[1] for g in got], [g[0] for g in got]
    offsets = np.zeros(len(records) + 1, np.int64)
    np.cumsum([len(b) for b in replies], out=offsets[1:])
    totals = np.array([kinds.count(ENCODED), int(offsets[-1]), kinds.count(DEFERRED), -1], np.int64)
    return replies, np.array(kinds, np.uint8), offsets, totals

