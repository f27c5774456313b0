"""fpx_wire_epx_classify_dev and fpx_wire_epx_replica_tick: a replica's inbox from wire bytes.  Bursts come from
tests/epaxos_inbox_mk_streams.make_burst; the model key k travels as the string b"k%d" % k inside a hand-assembled
CommandOrNoop (tests/epaxos_cmd_cases.py) that wire.epaxos_encode wraps into a ReplicaInbound frame.  The tick on context A
is held against context B, which goes the way the parent commit offers for the same frames -- the folded host decoder, the
classify written in Python with a dict for the ids, fpx_epx_replica_inbox_mk -- on every output, on the command logs and
index rows, and on the key table; and against InboxMkModel driven one message at a time."""
import numpy as np
import pytest

from tests import epaxos_cmd_cases as CC
from tests.epaxos_cluster import KINDS, command_of, frame  # noqa: F401  (shared with the cluster tests; imported from here too)
from tests import epaxos_inbox_mk_model as MM
from tests import epaxos_inbox_mk_streams as MS
from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_streams as S

pytestmark = pytest.mark.gpu
NK, NI = 4, 64
EINVAL, ECAPACITY = 1, 5


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def ctx(n, keys=True, num_keys=NK, arena=1 << 12):
    from frankenpaxos_amd.epaxos import EPaxos

    e = EPaxos(n, num_keys, num_instances=NI)
    if keys:
        e.keys_enable(arena)
    return e


def wire_burst(seed, n, m, **kw):
    """a burst as it can travel: an Accept or a Commit always carries its dependencies (the by-id form has no bytes)"""
    out = []
    for x in MS.make_burst(seed, n, m, num_keys=NK, num_instances=NI, **kw):
        if x[0] in (IM.IN_ACCEPT, IM.IN_COMMIT) and x[9][0] == -1:
            x = x[:9] + ([0] * n, 0)
        out.append(x)
    return out


def parent_way(wire, e, d, frames, to, triple):
    """context B: decode on the host, classify in Python, ids from the dict, fpx_epx_replica_inbox_mk"""
    dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=e.n)
    assert dec["status_code"] == 0
    buf = dec["buf"]
    cmds = [None if n < 0 else buf[o:o + n].tobytes() for o, n in zip(dec["cmd_off"], dec["cmd_len"])]
    cl = CC.classify(cmds)
    assert all(s != 0 for s in cl["cmd_shape"])
    ids = d.intern(cl["keys"])
    lists = [ids[cl["key_offsets"][i]:cl["key_offsets"][i + 1]] for i in range(len(frames))]
    kind = [KINDS[int(k)] for k in dec["kind"]]
    return e.replica_inbox_mk(kind, to, dec["instance_leader"], dec["instance_number"], dec["ballot_ordering"],
                              dec["ballot_replica"], lists, cl["is_set"], triple, dec["deps_watermark"], dec["deps_values_end"]), lists


def state(e, msgs, raw=True):
    return S.gpu_state(e, MS.cells_of(msgs), MS.all_keys(NK), raw=raw)


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("m", [1, 64, 65, 700])
def test_the_tick_equals_the_parent_way_and_the_model(wire, n, m):
    msgs = wire_burst(200 + m, n, m)
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    a, b, d = ctx(n), ctx(n, keys=False), CC.KeyDict()
    got = a.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)
    want, lists = parent_way(wire, b, d, frames, to, triple)
    assert got[0] == want[0] == 0
    for g, w in zip(got[1:7], want[1:]):
        np.testing.assert_array_equal(g, w)
    assert got[7:] == (-1, sum(len(x) for x in lists))
    assert state(a, msgs) == state(b, msgs)
    assert a.keys_read() == d.order()
    # ... and the model, one message at a time, under the ids the table gave
    model = MM.InboxMkModel(n, NK, NI)
    renamed = [x[:6] + (tuple(ks),) + x[7:] for x, ks in zip(msgs, lists)]
    rows = S.decode_outputs(n, renamed, got[1:7])
    for i, x in enumerate(renamed):
        st, r = model.inbox([x])
        assert st == IM.OK and rows[i] == tuple(r[0]), (i, x)
    cells = MS.cells_of(msgs)
    assert S.gpu_state(a, cells, MS.all_keys(NK)) == S.model_state(model, cells, MS.all_keys(NK))
    a.close(), b.close()


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("m", [1, 64, 65, 700])
def test_classify_dev_equals_the_host_classify_and_the_dict(wire, n, m):
    msgs = wire_burst(300 + m, n, m)
    cmds = [None if x[0] == IM.IN_PREPARE else command_of(x) for x in msgs]
    if m >= 64:                                                  # shape-0 commands are reported, not refused
        cmds[5] = CC.command(CC.get_request([b"k1"]) + CC.get_request([b"k2"]))
        cmds[40] = CC.get([b"k0"]) + CC.NOOP
    off, ln, at = [], [], 0
    for c in cmds:
        off.append(-1 if c is None else at), ln.append(-1 if c is None else len(c))
        at += 0 if c is None else len(c)
    buf = np.frombuffer(b"".join(c for c in cmds if c is not None) or b"\x00", np.uint8)
    host = wire.epx_classify(buf, off, ln)
    want = CC.classify(cmds)
    assert host["status_code"] == 0 and host["keys"] == want["keys"]
    e, d = ctx(n), CC.KeyDict()
    d.intern([b"k3"])
    assert e.keys_intern([b"k3"])[0] == 0                          # one key resident before the call
    before = len(d.order())
    ids = d.intern(want["keys"])
    P = len(ids)
    got = e.wire_classify_dev(buf, off, ln, max_pairs=P)
    assert got["status_code"] == 0
    for k in ("key_offsets", "is_set", "is_noop", "cmd_shape"):
        assert got[k].tolist() == list(host[k]) == want[k], k
    assert got["keys"].tolist() == ids
    new = d.order()[before:]
    assert got["result"].tolist() == [-1, P, len(new), sum(len(k) for k in new)]
    assert e.keys_read() == d.order()
    if P > 0:                                                    # one pair too few: refused, nothing interned
        e2 = ctx(n)
        got = e2.wire_classify_dev(buf, off, ln, max_pairs=P - 1)
        assert got["status_code"] == ECAPACITY and got["result"][1] == P and e2.keys_count() == (0, 0)
        e2.close()
    e.close()


def test_classify_dev_across_rows_of_the_scan(wire):
    """more than 2 048 commands and their pairs run over several rows of 1 024 of the two-level scan, the last one partly filled"""
    cmds = CC.seeded_burst(77, 2400)
    cmds = [c for c in cmds if c is None or CC.parse_command(c) != CC.MALFORMED]
    want = CC.classify(cmds)
    assert len(cmds) > 2048 and len(want["keys"]) > 2048
    off, ln, at = [], [], 0
    for c in cmds:
        off.append(-1 if c is None else at), ln.append(-1 if c is None else len(c))
        at += 0 if c is None else len(c)
    buf = np.frombuffer(b"".join(c for c in cmds if c is not None), np.uint8)
    e, d = ctx(3, num_keys=64, arena=1 << 13), CC.KeyDict()
    ids = d.intern(want["keys"])
    got = e.wire_classify_dev(buf, off, ln, max_pairs=len(ids) + 5)
    assert got["status_code"] == 0
    for k in ("key_offsets", "is_set", "is_noop", "cmd_shape"):
        assert got[k].tolist() == want[k], k
    assert got["keys"].tolist() == ids and e.keys_read() == d.order()
    e.close()


def test_a_malformed_command_refuses_the_classify(wire):
    cmds = [CC.get([b"a"]), CC.set_([b"b"])[:-1], CC.NOOP, b"\x0b"]
    off = np.cumsum([0] + [len(c) for c in cmds[:-1]])
    buf = np.frombuffer(b"".join(cmds), np.uint8)
    e = ctx(3)
    got = e.wire_classify_dev(buf, off, [len(c) for c in cmds], max_pairs=8)
    assert got["status_code"] == EINVAL and got["result"][0] == 1 and e.keys_count() == (0, 0)
    got = e.wire_classify_dev(buf, off[:1], [len(cmds[0])], max_pairs=8)          # and the context is fit for the next call
    assert got["status_code"] == 0 and got["keys"].tolist() == [0] and e.keys_read() == [b"a"]
    e.close()


def test_a_burst_cut_in_two_ticks_is_one_tick(wire):
    n, m = 5, 600
    msgs = wire_burst(41, n, m)
    frames = [frame(wire, x) for x in msgs]
    to, triple = [x[1] for x in msgs], [x[8] for x in msgs]
    whole = ctx(n)
    want = whole.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)
    assert want[0] == 0
    for cut in (1, 257, 599):
        halves = ctx(n)
        g1 = halves.wire_replica_tick(frames[:cut], to[:cut], max_pairs=5 * m, triple_id=triple[:cut])
        g2 = halves.wire_replica_tick(frames[cut:], to[cut:], max_pairs=5 * m, triple_id=triple[cut:])
        assert g1[0] == g2[0] == 0
        for w, x, y in zip(want[1:7], g1[1:7], g2[1:7]):
            np.testing.assert_array_equal(w, np.concatenate([x, y]))
        assert g1[8] + g2[8] == want[8]
        assert state(halves, msgs) == state(whole, msgs)
        assert halves.keys_read() == whole.keys_read()           # first occurrence in the stream is first occurrence in a cut
        halves.close()
    whole.close()


def test_prepares_only_and_the_default_triple_ids(wire):
    n = 5
    msgs = [x for x in wire_burst(52, n, 400) if x[0] == IM.IN_PREPARE][:70]
    assert len(msgs) > 40
    a, b = ctx(n), ctx(n, keys=False)
    frames, to = [frame(wire, x) for x in msgs], [x[1] for x in msgs]
    got = a.wire_replica_tick(frames, to, max_pairs=0)
    want, _ = parent_way(wire, b, CC.KeyDict(), frames, to, [-1] * len(msgs))
    assert got[0] == 0 and got[7:] == (-1, 0) and a.keys_count() == (0, 0)
    for g, w in zip(got[1:7], want[1:]):
        np.testing.assert_array_equal(g, w)
    # triple_id NULL: triple_base + i, and -1 for a Prepare
    msgs = wire_burst(53, n, 120)
    frames, to = [frame(wire, x) for x in msgs], [x[1] for x in msgs]
    triple = [-1 if x[0] == IM.IN_PREPARE else 7000 + i for i, x in enumerate(msgs)]
    got = a.wire_replica_tick(frames, to, max_pairs=600, triple_base=7000)
    want, _ = parent_way(wire, b, CC.KeyDict(), frames, to, triple)
    assert got[0] == 0
    for g, w in zip(got[1:7], want[1:]):
        np.testing.assert_array_equal(g, w)
    assert state(a, msgs) == state(b, msgs)
    a.close(), b.close()


def test_refusals_leave_the_state_and_the_key_table(wire):
    n = 5
    e = ctx(n, num_keys=NK + 1)                                   # (room for one key beyond the bursts' four)
    first = wire_burst(60, n, 100)
    assert e.wire_replica_tick([frame(wire, x) for x in first], [x[1] for x in first], max_pairs=500)[0] == 0
    msgs = wire_burst(61, n, 64, first_triple=5000)
    # a key the table does not hold yet in every refused burst: a refusal that interned it would show in keys_count
    fresh = CC.get([b"never seen"])
    frames = [frame(wire, x, command=fresh if i == 2 and x[0] != IM.IN_PREPARE else None) for i, x in enumerate(msgs)]
    if msgs[2][0] == IM.IN_PREPARE:
        frames[2] = frame(wire, (IM.IN_COMMIT,) + msgs[2][1:9] + ([0] * n, 0), command=fresh)
    to = [x[1] for x in msgs]
    before = (state(e, first + msgs), e.keys_count(), e.keys_read())
    pairs = 5 * 64

    def refused(frames, status, bad, offsets=None, max_pairs=pairs, to=to):
        got = e.wire_replica_tick(frames, to, max_pairs=max_pairs, offsets=offsets)
        assert (got[0], got[7]) == (status, bad)
        assert all((o == -9).all() for o in got[1:7])
        assert (state(e, first + msgs), e.keys_count(), e.keys_read()) == before
        return got

    z = [0] * n
    ok_frame = wire.epaxos_encode(17, (1, 2), ballot=(0, 1), replica_index=2, sequence_number=0, deps=z)     # a PreAcceptOk
    with_shape0 = list(frames)
    with_shape0[37] = frame(wire, (IM.IN_COMMIT, 0, 1, 2, 0, 0, (1,), 0, 9, z, 0), command=CC.get([b"k1"]) + CC.NOOP)
    refused(with_shape0, EINVAL, 37)
    other = list(frames)
    other[11] = ok_frame
    refused(other, EINVAL, 11)
    both = list(other)
    both[20] = with_shape0[37]
    refused(both, EINVAL, 11)                                     # the lowest offending index
    # deps_shape 0: an explicit id of another leader's column
    foreign = list(frames)
    foreign[50] = wire.epaxos_encode(18, (1, 2), ballot=(0, 1), command=CC.get([b"k1"]), sequence_number=0, deps=z, values=[(3, 9)])
    assert wire.epaxos_decode_replica_inbound_folded([foreign[50]], num_replicas=n)["deps_shape"][0] == 0
    refused(foreign, EINVAL, 50)
    # a malformed command inside a well-formed frame
    inner = list(frames)
    inner[8] = frame(wire, (IM.IN_COMMIT, 0, 1, 2, 0, 0, (1,), 0, 9, z, 0), command=CC.get([b"k1"]) + b"\x0b")
    refused(inner, EINVAL, 8)
    # a bad offset beside a malformed frame: the offset wins
    trunc = frames[:5] + [frames[5][:-2]] + frames[6:]
    off = np.cumsum([0] + [len(x) for x in trunc]).astype(np.int64)
    refused(trunc, EINVAL, 5)
    off[50] = off[49] - 3
    want = wire.epaxos_decode_replica_inbound_folded(trunc, num_replicas=n, offsets=off)["bad_index"]
    assert want > 5
    refused(trunc, EINVAL, want, offsets=off)
    # one pair too few
    need = e.wire_replica_tick(frames, to, max_pairs=pairs)
    assert need[0] == 0 and need[8] > 3
    e.close()

    e = ctx(n, num_keys=NK + 1)                                   # (the good tick above applied: a fresh context)
    assert e.wire_replica_tick([frame(wire, x) for x in first], [x[1] for x in first], max_pairs=500)[0] == 0
    got = refused(frames, ECAPACITY, -1, max_pairs=need[8] - 1)
    assert got[8] == need[8]
    # a burst that stage 1 accepts and the inbox refuses: no index, the logs untouched, the keys of the burst interned
    logs = state(e, first + msgs)
    got = e.wire_replica_tick(frames, [n] + to[1:], max_pairs=pairs)
    assert (got[0], got[7]) == (EINVAL, -1) and all((o == -9).all() for o in got[1:7])
    assert state(e, first + msgs) == logs
    assert e.keys_count()[0] == before[1][0] + 1 and e.keys_read()[-1] == b"never seen"
    outside = list(frames)
    outside[9] = wire.epaxos_encode(21, (1, NI), ballot=(0, 1))   # an instance outside the log
    got = e.wire_replica_tick(outside, to, max_pairs=pairs)
    assert (got[0], got[7]) == (EINVAL, -1) and state(e, first + msgs) == logs
    assert e.wire_replica_tick(frames, to, max_pairs=pairs)[0] == 0   # and the context is fit for the next tick
    e.close()


def test_the_tick_needs_the_key_table(wire):
    n = 3
    e = ctx(n, keys=False)
    msgs = wire_burst(70, n, 10)
    got = e.wire_replica_tick([frame(wire, x) for x in msgs], [x[1] for x in msgs], max_pairs=50)
    assert got[0] == EINVAL
    e.keys_enable(256)
    assert e.wire_replica_tick([], [], max_pairs=0)[0] == 0       # m = 0
    assert e.wire_replica_tick([frame(wire, x) for x in msgs], [x[1] for x in msgs], max_pairs=50)[0] == 0
    e.close()


def test_the_device_form_equals_the_host_form(wire):
    import torch

    n, m = 5, 300
    msgs = wire_burst(80, n, m)
    frames = [frame(wire, x) for x in msgs]
    to = np.asarray([x[1] for x in msgs], np.int32)
    host, dev = ctx(n), ctx(n)
    want = host.wire_replica_tick(frames, to, max_pairs=5 * m, triple_base=100)
    assert want[0] == 0
    buf, off = wire.pack(frames)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(5)]
    odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
    res = torch.full((2,), -9, dtype=torch.int32, device="cuda")
    dev.wire_replica_tick_dev(T(buf), len(buf), T(off), T(to), 5 * m, triple_base=100, outcome=outs[0], out_ballot=outs[1],
                              out_status=outs[2], out_deps=odeps, out_values_end=outs[3], out_triple=outs[4],
                              bad_index=res[0:1], num_pairs=res[1:2])
    assert dev.sync() == 0
    for g, w in zip([outs[0], outs[1], outs[2], odeps, outs[3], outs[4]], want[1:7]):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    assert tuple(res.cpu().numpy()) == want[7:]
    assert state(dev, msgs) == state(host, msgs) and dev.keys_read() == host.keys_read()
    host.close(), dev.close()
