"""The replica ticks on a context with the command store (fpx_epx_cmds_*, include/fpx_wire.h "with the command store"): twin
contexts get the same frames -- A has the store, B has none, and B's deferred replies are built on the host from the test's own
command list (first stored wins) by the host encoder, which tests/test_epaxos_cmd_reply_encode_cpu.py holds against the
yardstick.  Every reply must be byte-equal, the command logs equal, and on A nothing stays deferred but what the store cannot
answer.  The census of one hand-written burst is asserted record by record.  The streams of the inbox generators are played in
one burst and in two; their census -- the reply kind of every message, the counts, the classes of command replies -- is
computed on the CPU by the model before any GPU call and asserted exactly.  The model is epaxos_inbox_mk_model.py, the
multi-key restatement of epaxos_inbox_model.py (whose outcome constants and rows it shares): frames carry key lists, which the
single-key model cannot take."""
import numpy as np
import pytest

from tests import epaxos_inbox_model as IM
from tests.test_gpu_epaxos_wire_replica_tick import command_of, ctx, frame, state, wire_burst

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = 1, 5
MAX_TRIPLES = 1 << 12
SOA = ("outcome", "out_ballot", "out_status", "out_deps", "out_values_end", "out_triple")


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def with_store(n, arena=1 << 20):
    e = ctx(n)
    e.cmds_enable(MAX_TRIPLES, arena)
    return e


class Commands:
    """the test's own command list: triple id -> the first command a frame carried under it, as the plain arrays of the host
    encoder"""

    def __init__(self):
        self.by_id = {}

    def add(self, msgs):
        for x in msgs:
            if x[0] != IM.IN_PREPARE and 0 <= x[8] < MAX_TRIPLES:
                self.by_id.setdefault(x[8], command_of(x))

    def arrays(self):
        off, ln, arena = np.full(MAX_TRIPLES, -1, np.int64), np.zeros(MAX_TRIPLES, np.int32), bytearray()
        for t, c in self.by_id.items():
            off[t], ln[t] = len(arena), len(c)
            arena += c
        return off, ln, np.frombuffer(bytes(arena) or b"\0", np.uint8)

    def stats(self):
        return len(self.by_id), sum(len(c) for c in self.by_id.values())


def host_replies(wire, n, frames, to, soa, store, cap=None):
    """the host encoder on the decoded frames and a tick's struct-of-arrays outputs, with the command list (None: without)"""
    dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=n)
    assert dec["status_code"] == 0
    return wire.epx_encode_replica_replies_cmds(
        n, soa[5], store, cap=cap, to=to, leader=dec["instance_leader"], number=dec["instance_number"],
        ballot_ordering=dec["ballot_ordering"], ballot_replica=dec["ballot_replica"], outcome=soa[0], out_ballot=soa[1],
        out_status=soa[2], out_deps=soa[3], out_values_end=soa[4]), dec


def play(wire, n, a, b, cmds, msgs):
    """one burst on both: A's bytes tick against B's tick and the host encoder; -> (A's dict, B's tuple, the host's dict)"""
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    cmds.add(msgs)                                          # (the burst's own commands answer the burst's own Prepares)
    twin = b.wire_replica_tick(frames, to, max_pairs=5 * len(msgs), triple_id=triple)
    want, _ = host_replies(wire, n, frames, to, twin[1:7], cmds.arrays())
    cap = int(want["totals"][1]) + 16
    got = a.wire_replica_tick_bytes(frames, to, max_pairs=5 * len(msgs), triple_id=triple, out_cap=cap)
    assert got["status_code"] == twin[0] == want["status_code"] == 0
    for k, w in zip(SOA, twin[1:7]):
        np.testing.assert_array_equal(got[k], w)
    assert np.array_equal(got["totals"], want["totals"])
    assert np.array_equal(got["out_offsets"], want["out_offsets"]) and np.array_equal(got["reply_kind"], want["reply_kind"])
    assert got["replies"] == want["replies"]
    assert (got["out"][int(want["totals"][1]):] == 0xEE).all()
    assert a.cmds_stats() == cmds.stats() + (0, 0)
    return got, twin, want


def carries(twin, i):
    return twin[1][i] == 8 or (twin[1][i] == 6 and twin[3][i] in (2, 3))


def test_one_burst_reaches_every_reply_with_a_command(wire):
    """a short history at replica 0 -- a committed instance, a pre-accepted and an accepted entry, a committed Noop -- and a
    burst that meets each of them, with a Commit and a Prepare of one instance inside the burst"""
    n = 3
    z = [0] * n
    P, A, C, R = IM.IN_PRE_ACCEPT, IM.IN_ACCEPT, IM.IN_COMMIT, IM.IN_PREPARE
    history = [(C, 0, 1, 0, 0, 1, (0,), 1, 100, z, 0), (P, 0, 1, 1, 5, 1, (1,), 1, 101, z, 0), (A, 0, 1, 2, 5, 1, (2,), 0, 102, z, 0),
               (C, 0, 1, 3, 0, 1, (), 0, 99, z, 0)]          # (no keys and an id that is 0 mod 3: a Noop)
    burst = [(P, 0, 1, 0, 1, 1, (0,), 1, 200, z, 0),        # committed here: the Commit goes back to a PreAccept
             (A, 0, 1, 0, 1, 1, (0,), 1, 201, z, 0),        # ... to an Accept
             (R, 0, 1, 0, 9, 2, (), 0, -1, z, 0),           # ... to a Prepare
             (R, 0, 1, 1, 9, 2, (), 0, -1, z, 0),           # PrepareOk with the pre-accepted triple
             (R, 0, 1, 2, 9, 2, (), 0, -1, z, 0),           # ... with the accepted one
             (R, 0, 1, 3, 9, 2, (), 0, -1, z, 0),           # the committed Noop goes back
             (C, 0, 1, 6, 0, 1, (2, 3), 1, 207, z, 0),      # learnt in this burst ...
             (R, 0, 1, 6, 9, 2, (), 0, -1, z, 0),           # ... and asked for in this burst: this burst's bytes
             (R, 0, 1, 7, 9, 2, (), 0, -1, z, 0),           # nothing known: PrepareOk, NotSeen
             (P, 0, 1, 8, 9, 2, (1,), 1, 208, z, 0)]        # a steady PreAcceptOk behind them
    assert command_of(history[3]) == bytes([0x12, 0x00])
    a, b, cmds = with_store(n), ctx(n), Commands()
    play(wire, n, a, b, cmds, history)
    got, twin, want = play(wire, n, a, b, cmds, burst)
    assert got["outcome"].tolist() == [8, 8, 8, 6, 6, 8, 5, 8, 6, 1]
    assert got["out_status"].tolist()[3:5] == [2, 3] and got["out_status"][8] == 0
    assert got["reply_kind"].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1] and list(got["totals"][[0, 2, 3]]) == [9, 0, -1]
    # B, without the store, defers exactly the replies with a command
    plain, _ = host_replies(wire, n, [frame(wire, x) for x in burst], [x[1] for x in burst], twin[1:7], None)
    assert plain["reply_kind"].tolist() == [2, 2, 2, 2, 2, 2, 0, 2, 1, 1]
    # the replies parse as what the reference would have sent, and carry the stored bytes
    dec = wire.epaxos_decode_replica_inbound(got["replies"][:6] + got["replies"][7:], max_replicas=n)
    assert dec["status_code"] == 0
    assert dec["kind"].tolist() == [wire.EPX_COMMIT] * 3 + [wire.EPX_PREPARE_OK] * 2 + [wire.EPX_COMMIT] * 2 + \
        [wire.EPX_PREPARE_OK, wire.EPX_PRE_ACCEPT_OK]
    assert dec["status"].tolist()[3:5] == [1, 2] and dec["status"][7] == 0
    sent = [dec["buf"][o:o + k].tobytes() for o, k in zip(dec["cmd_off"], dec["cmd_len"])]
    assert sent[:7] == [command_of(x) for x in (history[0], history[0], history[0], history[1], history[2], history[3], burst[6])]
    assert dec["is_noop"].tolist()[5] == 1
    assert state(a, history + burst) == state(b, history + burst)
    a.close(), b.close()


CLASSES = {("back", IM.IN_PRE_ACCEPT), ("back", IM.IN_ACCEPT), ("back", IM.IN_PREPARE), ("ok", 2), ("ok", 3), "noop", "one burst"}


def model_census(n, parts):
    """what epaxos_inbox_mk_model.py says of the stream, on the CPU: per message the reply kind a context with the store must
    give, and the classes of command replies that occur.  A reply with a command is planned as deferred only where its
    dependencies are known by id alone or the own column has more than 64 explicit ids.  Neither can be in these streams: a
    frame cannot carry by-id dependencies (wire_burst), and the instance numbers stay below NI = 64.  So the plan is that NO
    command reply stays deferred; what is deferred is the PrepareOks of out_status 1, as on every context."""
    from tests import epaxos_inbox_mk_model as MM
    from tests.test_gpu_epaxos_wire_replica_tick import NI, NK

    model = MM.InboxMkModel(n, NK, NI)
    first, kinds, classes = {}, [], set()
    for part in parts:
        learnt = {}                                             # (to, instance) -> the triple a Commit of THIS burst brought
        for x in part:
            if x[0] != IM.IN_PREPARE:
                first.setdefault(x[8], x)
            st, rows = model.inbox([x])
            assert st == IM.OK
            outcome, _, status, deps, triple = rows[0]
            if outcome in (IM.RI_IGNORED, IM.RI_LEARNT):
                kind = 0
            elif outcome in (IM.RI_ACCEPT_OK, IM.RI_ACCEPT_OK_AGAIN, IM.RI_NACK) or (outcome == IM.RI_PREPARE_OK and status == 0):
                kind = 1
            elif outcome in (IM.RI_PRE_ACCEPT_OK, IM.RI_PRE_ACCEPT_OK_AGAIN):
                assert deps is not None
                kind = 1
            elif outcome == IM.RI_COMMIT_BACK or status in (2, 3):
                assert deps is not None and triple in first     # (the plan: nothing by id, every triple came in a frame)
                kind = 1
                classes.add(("back", x[0]) if outcome == IM.RI_COMMIT_BACK else ("ok", status))
                if command_of(first[triple]) == bytes([0x12, 0x00]):
                    classes.add("noop")
                if outcome == IM.RI_COMMIT_BACK and x[0] == IM.IN_PREPARE and learnt.get((x[1], x[2], x[3])) == triple:
                    classes.add("one burst")
            else:
                kind = 2                                        # a PrepareOk of out_status 1
            if x[0] == IM.IN_COMMIT and outcome == IM.RI_LEARNT:
                learnt[(x[1], x[2], x[3])] = x[8]
            kinds.append(kind)
    return kinds, classes


@pytest.mark.parametrize("n,seed,cut", [(3, 1200, None), (3, 1200, 130), (5, 1201, None), (5, 1201, 130)])
def test_streams_in_one_burst_and_in_two(wire, n, seed, cut):
    """the seeds are those for which the model alone, on the CPU, shows every class of CLASSES in one burst and in two"""
    m = 300
    msgs = wire_burst(seed, n, m)
    parts = [msgs] if cut is None else [msgs[:cut], msgs[cut:]]
    want_kinds, classes = model_census(n, parts)
    assert classes == CLASSES, classes
    a, b, cmds = with_store(n), ctx(n), Commands()
    kinds, deferred, encoded = [], 0, 0
    for part in parts:
        got, twin, want = play(wire, n, a, b, cmds, part)
        kinds += got["reply_kind"].tolist()
        encoded, deferred = encoded + int(got["totals"][0]), deferred + int(got["totals"][2])
        assert not any(carries(twin, i) and got["reply_kind"][i] != 1 for i in range(len(part)))
    # the census, exactly: every kind per message, the counts, and on A no command reply among the deferred
    assert kinds == want_kinds
    assert (encoded, deferred) == (want_kinds.count(1), want_kinds.count(2))
    assert state(a, msgs) == state(b, msgs)
    a.close(), b.close()


def test_a_refused_burst_stores_nothing_and_capacity_then_re_encode(wire):
    n, m = 3, 200
    msgs = wire_burst(1311, n, m)
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    a, b, cmds = with_store(n), ctx(n), Commands()
    # a frame the tick refuses: nothing applied, nothing stored
    bad = frames[:50] + [b"\x12\x03\x0a\x01"] + frames[50:]
    got = a.wire_replica_tick_bytes(bad, to[:50] + [0] + to[50:], max_pairs=5 * m, triple_id=triple[:50] + [7] + triple[50:])
    assert got["status_code"] == EINVAL and got["bad_index"] == 50 and a.cmds_stats() == (0, 0, 0, 0)
    # the encoder's FPX_ECAPACITY: the tick WAS applied and the commands are stored; the caller re-encodes with _cmds_dev
    cmds.add(msgs)
    twin = b.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)
    want, dec = host_replies(wire, n, frames, to, twin[1:7], cmds.arrays())
    need = int(want["totals"][1])
    assert want["totals"][0] > 0 and any(carries(twin, i) and want["reply_kind"][i] == 1 for i in range(m))
    got = a.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_id=triple, out_cap=need - 1)
    assert got["status_code"] == ECAPACITY and list(got["totals"]) == list(want["totals"])
    for k, w in zip(SOA, twin[1:7]):
        np.testing.assert_array_equal(got[k], w)
    assert a.cmds_stats() == cmds.stats() + (0, 0) and state(a, msgs) == state(b, msgs)
    again = a.encode_replica_replies(
        out_triple=got["out_triple"], to=to, leader=dec["instance_leader"], number=dec["instance_number"],
        ballot_ordering=dec["ballot_ordering"], ballot_replica=dec["ballot_replica"], outcome=got["outcome"],
        out_ballot=got["out_ballot"], out_status=got["out_status"], out_deps=got["out_deps"], out_values_end=got["out_values_end"])
    assert again["status_code"] == 0 and again["replies"] == want["replies"]
    assert np.array_equal(again["reply_kind"], want["reply_kind"]) and np.array_equal(again["totals"], want["totals"])
    # the plain tick puts as well
    c = with_store(n)
    assert c.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)[0] == 0
    assert c.cmds_stats() == a.cmds_stats() and [c.cmds_read(t) for t in cmds.by_id] == list(cmds.by_id.values())
    a.close(), b.close(), c.close()
