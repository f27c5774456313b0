"""EPaxos ReplicaInbound messages decoded on the device (fpx_wire_epaxos_decode_replica_inbound_dev) and a leader's tick from
wire bytes to decisions (fpx_wire_epx_leader_tick), include/fpx_wire.h.  The device decoder must equal the folded host
decoder array for array (which tests/test_epaxos_wire_folded_cpu.py holds against the existing decoder); the tick must leave
every output and every piece of device state as fpx_epx_leader_replies leaves them on the host-decoded arrays, and as
tests/epaxos_leader_model.py says."""
import numpy as np
import pytest

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as S
from tests import epaxos_wire_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def ctx(n, num_keys=4, num_instances=64, leader_state=True):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, num_keys, num_instances=num_instances, leader_state=leader_state)


_pools = {}


def pool(wire, n):
    """the fold edge cases, then generated messages of every kind: one list per n, made once"""
    if n not in _pools:
        _pools[n] = [c[1] for c in W.edge_cases(n)] + W.generated_burst(wire, 30 + n, n, 257)
    return _pools[n]


# ---- device decode == folded host decode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [3, 5, 7])
def test_device_decode_equals_the_folded_host_decode(wire, n, m):
    p = pool(wire, n)
    msgs = p[1:2] if m == 1 else (p[:m] if m < 257 else p[-257:])     # (m = 1: a PreAcceptOk with an explicit id)
    want = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n)
    assert want["status_code"] == 0
    e = ctx(n)
    got = e.wire_decode_dev(msgs)
    assert got["status_code"] == 0 and got["bad_index"] == -1
    for k in wire.EPX_FOLDED_NAMES:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if m >= 63:
        assert {-1, 0, 1} <= set(want["deps_shape"].tolist())
    e.close()


@pytest.mark.parametrize("n", [3, 5, 7])
def test_device_decode_with_every_optional_array_left_out(wire, n):
    msgs = pool(wire, n)
    want = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n, only_kind=True)
    e = ctx(n)
    got = e.wire_decode_dev(msgs, only_kind=True)
    assert got["status_code"] == 0 and got["bad_index"] == -1 and sorted(got) == ["bad_index", "kind", "status_code"]
    np.testing.assert_array_equal(got["kind"], want["kind"])
    none = e.wire_decode_dev([])
    assert none["status_code"] == 0 and none["bad_index"] == -1
    e.close()


# ---- malformed input -----------------------------------------------------------------------------------------------------
def bad_ticks(wire, n):
    """[(name, messages, offsets or None)]"""
    good = pool(wire, n)[:70]
    trunc = good[3][:-2]
    lens = np.cumsum([0] + [len(x) for x in good]).astype(np.int64)
    out = [("truncated, first", [trunc] + good, None), ("truncated, in the middle", good[:66] + [trunc] + good[66:], None),
           ("truncated, last", good + [trunc], None)]
    down = lens.copy()
    down[40] = down[39] - 1
    out.append(("a decreasing offset", good, down))
    past = lens.copy()
    past[-1] += 1
    out.append(("the last offset past the buffer", good, past))
    msgs = good[:5] + [trunc] + good[5:]
    both = np.cumsum([0] + [len(x) for x in msgs]).astype(np.int64)
    both[50] = both[49] - 3
    out.append(("a malformed message, then a bad offset: the offset wins", msgs, both))
    for name, msg in W.malformed_cases(n):
        out.append((name, good[:64] + [msg], None))
    return out


@pytest.mark.parametrize("n", [3, 5])
def test_malformed_ticks_give_the_host_decoders_bad_index_and_einval_at_sync(wire, n):
    e = ctx(n)
    for name, msgs, off in bad_ticks(wire, n):
        want = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n, offsets=off)
        assert want["status_code"] == M.EINVAL and want["bad_index"] >= 0, name
        got = e.wire_decode_dev(msgs, offsets=off)
        assert (got["status_code"], got["bad_index"]) == (M.EINVAL, want["bad_index"]), name
        assert e.sync() == 0                                          # reported once
    # and the context decodes the next good tick
    msgs = pool(wire, n)[:70]
    got = e.wire_decode_dev(msgs)
    assert got["status_code"] == 0 and got["bad_index"] == -1
    np.testing.assert_array_equal(got["deps_shape"], wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n)["deps_shape"])
    e.close()


def test_a_call_enqueued_behind_a_failed_decode_applies_nothing(wire):
    import torch

    n, z = 5, [0] * 5
    e = ctx(n)
    assert e.lead([0], [0], [0], [0], [1], [1], [7])[0] == 0
    before = e.read_leader_state(0, 0, 0)
    reply = (M.PRE_ACCEPT_OK, 0, 0, 0, 0, 0, 1, 0, z, 0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    a = [T(x) for x in S.burst_arrays(n, [reply])]
    outcome = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    msgs = pool(wire, n)[:10] + [pool(wire, n)[2][:-1]]
    buf, off = wire.pack(msgs)
    d_buf, d_off = T(buf), T(off)
    torch.cuda.synchronize()
    t = e.wire_decode_dev_tensors(d_buf, int(off[-1]), d_off, len(msgs))
    e.leader_replies_dev(*a, outcome=outcome)
    assert e.sync() == M.EINVAL and int(t["bad_index"].item()) == 10
    after = e.read_leader_state(0, 0, 0)
    assert list(after[0]) == list(before[0]) and (after[1] == before[1]).all() and int(outcome.item()) == -9
    # the same call on its own does apply: the leader state has one more answer
    e.leader_replies_dev(*a, outcome=outcome)
    assert e.sync() == 0 and int(outcome.item()) == M.WAITING
    assert list(e.read_leader_state(0, 0, 0)[0]) != list(before[0])
    e.close()


# ---- the tick == decode + call -----------------------------------------------------------------------------------------------
def encode(wire, msg):
    kind, to, L, x, bo, br, q, seq, w, end = msg
    if kind == M.PRE_ACCEPT_OK:
        return wire.epaxos_encode(wire.EPX_PRE_ACCEPT_OK, (L, x), (bo, br), replica_index=q, sequence_number=seq, deps=w,
                                  values=[(L, y) for y in range(x + 1, end)][::-1])
    if kind == M.ACCEPT_OK:
        return wire.epaxos_encode(wire.EPX_ACCEPT_OK, (L, x), (bo, br), replica_index=q)
    assert kind == M.NACK
    return wire.epaxos_encode(wire.EPX_NACK, (L, x), (bo, br))


def cut_at_timers(ops):
    """every `replies` op cut into ops of wire messages only and ops of timer events only, in order"""
    out = []
    for op in ops:
        if op[0] != "replies":
            out.append(op)
            continue
        run = []
        for msg in op[1]:
            if run and (run[-1][0] == M.SLOW_PATH_TIMER) != (msg[0] == M.SLOW_PATH_TIMER):
                out.append(("replies", run))
                run = []
            run.append(msg)
        out.append(("replies", run))
    return out


def rows(n, st, outcome, oseq, odeps, oend, otr, dec):
    if st == M.EINVAL:
        return (st, None, None)
    m = len(outcome)
    return (st, [(int(outcome[i]), int(oseq[i]), [int(v) for v in odeps[i]], int(oend[i]), int(otr[i])) for i in range(m)],
            [int(v) for v in dec])


def host_decoded_arrays(wire, n, msgs, to):
    """the arrays of fpx_epx_leader_replies from the EXISTING host decoder, the fold done here (ownEnd of EPaxosNative.scala)"""
    d = wire.epaxos_decode_replica_inbound(msgs, max_replicas=n)
    assert d["status_code"] == 0
    kind = np.asarray([{17: 0, 19: 1, 23: 2}[int(k)] for k in d["kind"]], np.int32)
    ridx = np.where(kind == 2, 0, d["replica_index"]).astype(np.int32)     # a Nack carries none
    dend = np.zeros(len(msgs), np.int32)
    for i in range(len(msgs)):
        own = [int(v) for l, v in zip(d["values_leader"][d["values_off"][i]:d["values_off"][i + 1]],
                                      d["values_id"][d["values_off"][i]:d["values_off"][i + 1]]) if l == d["instance_leader"][i]]
        dend[i] = max(own) + 1 if own else 0
    return [kind, np.asarray(to, np.int32), d["instance_leader"], d["instance_number"], d["ballot_ordering"], d["ballot_replica"],
            ridx, d["sequence_number"], d["deps_watermark"], dend]


def play(wire, e, ops, tick):
    n, out = e.n, []
    for op in ops:
        if op[0] != "replies" or not op[1] or op[1][0][0] == M.SLOW_PATH_TIMER:
            out.append(S.run_gpu_op(e, op))
            continue
        msgs, to = [encode(wire, x) for x in op[1]], [x[1] for x in op[1]]
        if tick:
            res = e.wire_leader_tick(msgs, to)
            assert res[7] == -1
            out.append(rows(n, *res[:7]))
        else:
            out.append(rows(n, *e.leader_replies(*host_decoded_arrays(wire, n, msgs, to))))
    return out


def _ok(q, w, to=0, L=0, x=0, ballot=None, seq=0, end=0):
    ballot = (0, to) if ballot is None else ballot
    return (M.PRE_ACCEPT_OK, to, L, x, ballot[0], ballot[1], q, seq, list(w), end)


def streams(n):
    yield S.make_stream(1, n)
    yield [("lead", [(0, 0, 0, 0, 1, 1, 7, 0)]), ("replies", [_ok(q, [0] * n) for q in range(1, n)])]     # the quorum sizes
    # explicit ids on the wire (instance (0, 4), ids 5 .. 7 from one sender, a plain cover from another): a union on covers
    z = [0] * (n - 1)
    yield [("lead", [(0, 4, 0, 0, 0, 1, 9, 0)]),
           ("replies", [_ok(1, [4] + z, x=4, end=8), _ok(2, [5] + z, x=4)] + [_ok(q, [4] + z, x=4, end=6) for q in range(3, n)])]


@pytest.mark.parametrize("n", [3, 5, 7])
def test_the_tick_equals_decode_plus_call_and_the_model(wire, n):
    census = set()
    for ops in streams(n):
        ops = cut_at_timers(ops)
        a, b, model = ctx(n), ctx(n), M.LeaderModel(n, 4, 64)
        want = S.run_model(model, ops)
        via_call, via_tick = play(wire, a, ops, False), play(wire, b, ops, True)
        assert via_call == want
        assert via_tick == want
        step = 1 + len(S.touched(ops)[0]) // 128
        state = S.model_state(model, ops, step)
        assert S.gpu_state(a, ops, step) == state
        assert S.gpu_state(b, ops, step) == state
        for op, res in zip(ops, want):
            if op[0] == "replies":
                census.add(res[0])
                census.update(("outcome", r[0]) for r in res[1] or [])
                census.update(("end", r[3] > 0) for r in res[1] or [])
        a.close(), b.close()
    # the streams reach both status codes, every outcome of a wire message and explicit ids in a decision
    assert {0, M.EFATAL} <= census and ("end", True) in census
    assert {("outcome", k) for k in range(9) if (n, k) != (3, M.START_SLOW_PATH_TIMER)} <= census      # (n = 3 has no such timer)


# ---- what the tick refuses -----------------------------------------------------------------------------------------------------
def test_tick_refusals_apply_nothing_and_the_next_good_tick_applies(wire):
    n, z = 5, [0] * 5
    ops = [("lead", [(0, 2, 0, 0, 1, 1, 7, 0), (1, 0, 1, 0, 1, 0, 8, 0)]), ("replies", [_ok(1, z, x=2)])]
    e, model = ctx(n), M.LeaderModel(n, 4, 64)
    assert play(wire, e, ops, True) == S.run_model(model, ops)
    good, good2 = _ok(2, z, x=2), _ok(3, z, L=1, x=0, to=1)
    probe = ops + [("replies", [good, good2])]
    before = S.gpu_state(e, probe)
    assert before == S.model_state(model, probe)
    inst, bal = (0, 2), (0, 0)
    sets = lambda k, ids=(): [W.prefix_set(2 if l == 0 else 0, ids if l == 0 else ()) for l in range(k)]
    ok65 = W.pre_accept_ok(inst, bal, 2, 0, W.deps_body(sets(n, range(3, 3 + 65))))
    ok64 = W.pre_accept_ok(inst, bal, 2, 0, W.deps_body(sets(n, range(3, 3 + 64))))
    assert wire.epaxos_decode_replica_inbound_folded([ok65, ok64], n)["deps_shape"].tolist() == [0, 1]
    refused = [
        ("a PreAccept", wire.epaxos_encode(wire.EPX_PRE_ACCEPT, inst, bal, sequence_number=0, command=None, deps=z)),
        ("a PreAcceptOk with 65 ids", ok65),
        ("a PreAcceptOk with n - 1 sets", W.pre_accept_ok(inst, bal, 2, 0, W.deps_body(sets(n - 1)))),
        ("a PreAcceptOk with n + 1 sets", W.pre_accept_ok(inst, bal, 2, 0, W.deps_body(sets(n + 1)))),
        ("a truncated message", encode(wire, good)[:-1]),
        ("a PreAcceptOk with an id in a foreign column",
         wire.epaxos_encode(wire.EPX_PRE_ACCEPT_OK, inst, bal, replica_index=2, sequence_number=0, deps=z, values=[(1, 4)])),
        ("a Commit", wire.epaxos_encode(wire.EPX_COMMIT, inst, sequence_number=0, command=None, deps=z)),
        ("a Prepare", wire.epaxos_encode(wire.EPX_PREPARE, inst, bal)),
        ("a ClientRequest", W.CLIENT_REQUEST),
        ("an empty message", b""),
    ]
    for name, bad in refused:
        for at in (0, 1, 2):
            msgs = [encode(wire, good), encode(wire, good2)]
            msgs.insert(at, bad)
            to = [0, 1]
            to.insert(at, 0)
            st, outcome, oseq, odeps, oend, otr, dec, bad_index = e.wire_leader_tick(msgs, to)
            assert (st, bad_index) == (M.EINVAL, at), name
            assert (outcome == -9).all() and (oseq == -9).all() and (odeps == -9).all() and (oend == -9).all() and (otr == -9).all()
            assert len(dec) == 0
    # two offenders: the lowest index; a bad offset outranks both
    msgs = [encode(wire, good), refused[0][1], refused[4][1], encode(wire, good2)]
    assert e.wire_leader_tick(msgs, [0, 0, 0, 1])[::7] == (M.EINVAL, 1)
    off = np.cumsum([0] + [len(x) for x in msgs]).astype(np.int64)
    off[3] = off[2] - 1
    assert e.wire_leader_tick(msgs, [0, 0, 0, 1], offsets=off)[::7] == (M.EINVAL, 3)
    # a burst that decodes cleanly but that fpx_epx_leader_replies refuses: no index
    assert e.wire_leader_tick([encode(wire, good)], [n])[::7] == (M.EINVAL, -1)
    assert e.wire_leader_tick([encode(wire, _ok(2, z, x=64))], [0])[::7] == (M.EINVAL, -1)
    assert S.gpu_state(e, probe) == before
    # and the context still works: the next good tick applies
    tail = [("replies", [good, good2, _ok(3, z, x=2)])]
    assert play(wire, e, tail, True) == S.run_model(model, tail)
    assert S.gpu_state(e, probe + tail) == S.model_state(model, probe + tail)
    e.close()


def test_empty_tick_and_a_context_without_leader_state(wire):
    e = ctx(5)
    st, outcome, _, _, _, _, dec, bad = e.wire_leader_tick([], [])
    assert (st, bad) == (0, -1) and len(outcome) == 0 and len(dec) == 0
    e.close()
    e = ctx(5, leader_state=False)
    assert e.wire_leader_tick([wire.epaxos_encode(wire.EPX_NACK, (0, 0), (1, 1))], [0])[0] == M.EINVAL
    assert e.wire_decode_dev([wire.epaxos_encode(wire.EPX_NACK, (0, 0), (1, 1))])["kind"].tolist() == [wire.EPX_NACK]
    e.close()
