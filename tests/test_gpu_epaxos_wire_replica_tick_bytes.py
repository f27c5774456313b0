"""fpx_wire_epx_replica_tick_bytes: frames in, the frames to send back out.  The bytes tick against the existing tick on a twin
context fed the same frames (the generators of tests/test_gpu_epaxos_wire_replica_tick.py, multi-key commands): the reply bytes
are the host batch encoder's on the twin's struct-of-arrays outputs, the optional outputs and the command logs are equal, a
burst cut in two gives the concatenation, every refusal of the existing tick leaves state and outputs alone, and one burst
reaches every outcome, both deferred kinds among them."""
import numpy as np
import pytest

from tests import epaxos_cmd_cases as CC
from tests import epaxos_inbox_model as IM
from tests.test_gpu_epaxos_wire_replica_tick import NK, ctx, frame, state, wire_burst

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = 1, 5
SOA = ("outcome", "out_ballot", "out_status", "out_deps", "out_values_end", "out_triple")


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def host_replies(wire, n, frames, to, soa, cap=None):
    """the host batch encoder on the decoded frames and a tick's struct-of-arrays outputs (outcome, out_ballot, out_status,
    out_deps, out_values_end, ...)"""
    dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=n)
    assert dec["status_code"] == 0
    return wire.epx_encode_replica_replies(
        n, cap=cap, to=to, leader=dec["instance_leader"], number=dec["instance_number"], ballot_ordering=dec["ballot_ordering"],
        ballot_replica=dec["ballot_replica"], outcome=soa[0], out_ballot=soa[1], out_status=soa[2], out_deps=soa[3],
        out_values_end=soa[4])


def assert_bytes_tick(wire, n, got, twin, frames, to):
    """got: wire_replica_tick_bytes's dict; twin: wire_replica_tick's tuple on the same frames"""
    assert got["status_code"] == twin[0] == 0
    for k, w in zip(SOA, twin[1:7]):
        np.testing.assert_array_equal(got[k], w)
    assert (got["bad_index"], got["num_pairs"]) == twin[7:]
    want = host_replies(wire, n, frames, to, twin[1:7])
    assert want["status_code"] == 0 and np.array_equal(got["totals"], want["totals"])
    assert np.array_equal(got["out_offsets"], want["out_offsets"]) and np.array_equal(got["reply_kind"], want["reply_kind"])
    assert got["replies"] == want["replies"]
    need = int(want["totals"][1])
    assert (got["out"][need:] == 0xEE).all()
    return want


@pytest.mark.parametrize("n,m", [(3, 300), (5, 257), (5, 1)])
def test_the_bytes_tick_equals_the_tick_and_the_host_encoder(wire, n, m):
    msgs = wire_burst(900 + m, n, m)
    assert m == 1 or max(len(x[6]) for x in msgs) > 1                      # multi-key commands
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    a, b, c = ctx(n), ctx(n), ctx(n)
    twin = b.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)
    got = a.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_id=triple)
    want = assert_bytes_tick(wire, n, got, twin, frames, to)
    assert m == 1 or (want["totals"][0] > m // 2 and len(set(want["reply_kind"].tolist())) == 3)
    assert state(a, msgs) == state(b, msgs) and a.keys_read() == b.keys_read()
    # every struct-of-arrays output left out: the same bytes, from the tick's own scratch
    bare = c.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_id=triple, soa=False, out_cap=int(want["totals"][1]))
    assert bare["status_code"] == 0 and bare["replies"] == want["replies"] and np.array_equal(bare["totals"], want["totals"])
    assert np.array_equal(bare["reply_kind"], want["reply_kind"]) and state(c, msgs) == state(b, msgs)
    a.close(), b.close(), c.close()


def test_a_burst_cut_in_two_gives_the_concatenation(wire):
    n, m = 5, 400
    msgs = wire_burst(941, n, m)
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    whole = ctx(n)
    want = whole.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_id=triple)
    assert want["status_code"] == 0
    for cut in (1, 257):
        halves = ctx(n)
        g1 = halves.wire_replica_tick_bytes(frames[:cut], to[:cut], max_pairs=5 * m, triple_id=triple[:cut])
        g2 = halves.wire_replica_tick_bytes(frames[cut:], to[cut:], max_pairs=5 * m, triple_id=triple[cut:])
        assert g1["status_code"] == g2["status_code"] == 0
        assert g1["replies"] + g2["replies"] == want["replies"]
        assert np.array_equal(np.concatenate([g1["reply_kind"], g2["reply_kind"]]), want["reply_kind"])
        assert list(g1["totals"][:3] + g2["totals"][:3]) == list(want["totals"][:3])
        assert state(halves, msgs) == state(whole, msgs)
        halves.close()
    whole.close()


def test_one_burst_reaches_every_outcome(wire):
    """a short history at replica 0 -- a committed instance, a pre-accepted and an accepted entry, a NoCommandEntry in a high
    ballot -- and then a burst that meets each of them"""
    n = 3
    z = [0] * n
    P, A, C, R = IM.IN_PRE_ACCEPT, IM.IN_ACCEPT, IM.IN_COMMIT, IM.IN_PREPARE
    history = [(C, 0, 1, 0, 0, 1, (0,), 1, 100, z, 0), (P, 0, 1, 1, 5, 1, (1,), 1, 101, z, 0), (A, 0, 1, 2, 5, 1, (2,), 0, 102, z, 0),
               (R, 0, 1, 3, 9, 2, (), 0, -1, z, 0)]
    burst = [(P, 0, 1, 0, 1, 1, (0,), 1, 200, z, 0),        # committed here: the Commit goes back
             (P, 0, 1, 3, 1, 1, (3,), 1, 201, z, 0),        # an entry in a higher ballot: Nack
             (P, 0, 1, 1, 5, 1, (1,), 1, 202, z, 0),        # pre-accepted in this ballot: the PreAcceptOk again
             (P, 0, 1, 2, 5, 1, (2,), 0, 203, z, 0),        # accepted in this ballot: ignored
             (A, 0, 1, 2, 5, 1, (2,), 0, 204, z, 0),        # ... and the AcceptOk again
             (P, 0, 1, 4, 9, 2, (0, 1), 1, 205, z, 0), (A, 0, 1, 5, 9, 2, (1,), 0, 206, z, 0), (C, 0, 1, 6, 0, 1, (2, 3), 1, 207, z, 0),
             (R, 0, 1, 7, 9, 2, (), 0, -1, z, 0),           # nothing known: PrepareOk, NotSeen
             (R, 0, 1, 1, 9, 2, (), 0, -1, z, 0),           # PrepareOk with the pre-accepted triple: deferred
             (R, 0, 1, 2, 9, 2, (), 0, -1, z, 0),           # ... with the accepted one: deferred
             (R, 0, 1, 0, 9, 2, (), 0, -1, z, 0)]           # committed: deferred
    a, b = ctx(n), ctx(n)
    for e in (a, b):
        assert e.wire_replica_tick([frame(wire, x) for x in history], [x[1] for x in history], max_pairs=20,
                                   triple_id=[x[8] for x in history])[0] == 0
    frames, to, triple = [frame(wire, x) for x in burst], [x[1] for x in burst], [x[8] for x in burst]
    twin = b.wire_replica_tick(frames, to, max_pairs=40, triple_id=triple)
    got = a.wire_replica_tick_bytes(frames, to, max_pairs=40, triple_id=triple)
    want = assert_bytes_tick(wire, n, got, twin, frames, to)
    assert got["outcome"].tolist() == [8, 7, 2, 0, 4, 1, 3, 5, 6, 6, 6, 8]
    assert got["out_status"].tolist()[8:11] == [0, 2, 3]
    assert got["reply_kind"].tolist() == [2, 1, 1, 0, 1, 1, 1, 0, 1, 2, 2, 2] and list(got["totals"]) == [6, int(want["totals"][1]), 4, -1]
    # the replies parse as what the reference would have sent
    d = wire.epaxos_decode_replica_inbound([r for r in got["replies"] if r], max_replicas=n)
    assert d["status_code"] == 0 and d["kind"].tolist() == [23, 17, 19, 17, 19, 22]
    assert state(a, history + burst) == state(b, history + burst)
    a.close(), b.close()


def test_refusals_leave_state_and_outputs_alone(wire):
    n = 5
    e = ctx(n, num_keys=NK + 1)
    first = wire_burst(960, n, 100)
    assert e.wire_replica_tick([frame(wire, x) for x in first], [x[1] for x in first], max_pairs=500)[0] == 0
    msgs = wire_burst(961, n, 64, first_triple=5000)
    frames, to = [frame(wire, x) for x in msgs], [x[1] for x in msgs]
    before = (state(e, first + msgs), e.keys_count(), e.keys_read())
    pairs = 5 * 64

    def refused(frames, status, bad, offsets=None, max_pairs=pairs, to=to, keys_too=True):
        got = e.wire_replica_tick_bytes(frames, to, max_pairs=max_pairs, offsets=offsets)
        assert (got["status_code"], got["bad_index"]) == (status, bad)
        assert all((got[k] == -9).all() for k in SOA)
        assert list(got["totals"]) == [0, 0, 0, -1] and got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all()
        assert (got["reply_kind"] == 9).all() and (got["out"] == 0xEE).all() and got["replies"] == []
        assert state(e, first + msgs) == before[0]
        assert not keys_too or (e.keys_count(), e.keys_read()) == before[1:]
        return got

    z = [0] * n
    other = list(frames)
    other[11] = wire.epaxos_encode(17, (1, 2), ballot=(0, 1), replica_index=2, sequence_number=0, deps=z)     # a PreAcceptOk
    refused(other, EINVAL, 11)
    shape0 = list(other)
    shape0[7] = frame(wire, (IM.IN_COMMIT, 0, 1, 2, 0, 0, (1,), 0, 9, z, 0), command=CC.get([b"k1"]) + CC.NOOP)
    refused(shape0, EINVAL, 7)                                        # the lowest offending index
    trunc = frames[:5] + [frames[5][:-2]] + frames[6:]
    refused(trunc, EINVAL, 5)
    off = np.cumsum([0] + [len(x) for x in trunc]).astype(np.int64)
    off[50] = off[49] - 3
    bad = wire.epaxos_decode_replica_inbound_folded(trunc, num_replicas=n, offsets=off)["bad_index"]
    refused(trunc, EINVAL, bad, offsets=off)                          # a bad offset outranks a malformed frame
    need = e.wire_replica_tick_bytes(frames, to, max_pairs=pairs)
    assert need["status_code"] == 0 and need["num_pairs"] > 3
    e.close()

    e = ctx(n, num_keys=NK + 1)
    assert e.wire_replica_tick([frame(wire, x) for x in first], [x[1] for x in first], max_pairs=500)[0] == 0
    got = refused(frames, ECAPACITY, -1, max_pairs=need["num_pairs"] - 1)      # stage 1's FPX_ECAPACITY: nothing applied
    assert got["num_pairs"] == need["num_pairs"]
    refused(frames, EINVAL, -1, to=[n] + to[1:], keys_too=False)     # stage 1 accepts, the inbox refuses
    outside = list(frames)
    outside[9] = wire.epaxos_encode(21, (1, 64), ballot=(0, 1))       # an instance outside the log
    refused(outside, EINVAL, -1, keys_too=False)
    # the ENCODER's FPX_ECAPACITY: the tick WAS applied, the struct-of-arrays outputs are valid, the caller encodes from them
    twin = ctx(n, num_keys=NK + 1)
    assert twin.wire_replica_tick([frame(wire, x) for x in first], [x[1] for x in first], max_pairs=500)[0] == 0
    t = twin.wire_replica_tick(frames, to, max_pairs=pairs)
    want = host_replies(wire, n, frames, to, t[1:7])
    short = e.wire_replica_tick_bytes(frames, to, max_pairs=pairs, out_cap=int(want["totals"][1]) - 1)
    assert short["status_code"] == ECAPACITY and np.array_equal(short["totals"], want["totals"])
    for k, w in zip(SOA, t[1:7]):
        np.testing.assert_array_equal(short[k], w)
    assert short["out_offsets"][0] == 0 and (short["out_offsets"][1:] == -9).all() and (short["out"] == 0xEE).all()
    assert state(e, first + msgs) == state(twin, first + msgs)
    assert host_replies(wire, n, frames, to, [short[k] for k in SOA])["replies"] == want["replies"]
    # ... and the context is fit for the next tick
    more = wire_burst(962, n, 70, first_triple=7000)
    f2, to2 = [frame(wire, x) for x in more], [x[1] for x in more]
    assert_bytes_tick(wire, n, e.wire_replica_tick_bytes(f2, to2, max_pairs=400), twin.wire_replica_tick(f2, to2, max_pairs=400), f2, to2)
    e.close(), twin.close()


def test_the_empty_tick_and_the_device_form(wire):
    import torch

    n, m = 5, 130
    a, b = ctx(n), ctx(n)
    got = a.wire_replica_tick_bytes([], [], max_pairs=0)
    assert got["status_code"] == 0 and list(got["totals"]) == [0, 0, 0, -1] and list(got["out_offsets"]) == [0]
    msgs = wire_burst(970, n, m)
    frames, to = [frame(wire, x) for x in msgs], [x[1] for x in msgs]
    want = b.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_base=300)
    assert want["status_code"] == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    buf, off = wire.pack(frames)
    cap = m * wire.EPX_REPLY_MAX
    d_buf, d_off, d_to = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (buf, off, np.array(to, np.int32)))
    out = torch.full((cap,), 0xEE, dtype=torch.uint8, device=dev)
    ooff, kind = torch.full((m + 1,), -9, dtype=torch.int64, device=dev), torch.full((m,), 9, dtype=torch.uint8, device=dev)
    totals, bad = torch.full((4,), -9, dtype=torch.int64, device=dev), torch.full((1,), -9, dtype=torch.int32, device=dev)
    outcome = torch.full((m,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    a.wire_replica_tick_bytes_dev(d_buf, len(buf), d_off, d_to, 5 * m, out, cap, ooff, kind, totals, triple_base=300,
                                  outcome=outcome, bad_index=bad)
    assert a.sync() == 0 and bad.item() == -1
    assert np.array_equal(totals.cpu().numpy(), want["totals"]) and np.array_equal(ooff.cpu().numpy(), want["out_offsets"])
    assert np.array_equal(kind.cpu().numpy(), want["reply_kind"]) and np.array_equal(outcome.cpu().numpy(), want["outcome"])
    need = int(want["totals"][1])
    o = out.cpu().numpy()
    assert o[:need].tobytes() == want["out"][:need].tobytes() and (o[need:] == 0xEE).all()
    assert state(a, msgs) == state(b, msgs)
    a.close(), b.close()
