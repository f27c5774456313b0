"""fpx_epx_replica_inbox[_dev]: a burst of PreAccept / Accept / Commit / Prepare messages at hosted replicas in one device
call, against tests/epaxos_inbox_model.py (the set model of oracle/epaxos_sets.py, one message at a time) on every output --
dependencies compared as sets -- and on the command log, largestBallot and the conflict index read back through
fpx_epx_read_cmdlog[_deps] / fpx_epx_read_index; against the library's own per-kind entry points, one message per call, bit
for bit; and against itself with the burst cut in two.  tests/test_epaxos_inbox_cpu.py asserts what the bursts exercise."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_streams as S
from tests.test_epaxos_inbox_cpu import MODEL_BURSTS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock-JVM fixture)

pytestmark = pytest.mark.gpu
NK, NI = 4, 64


def ctx(n, num_instances=NI, leader_state=False):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, NK, num_instances=num_instances, leader_state=leader_state)


def run(e, msgs):
    """(status, the outputs decoded into the model's rows, the raw output arrays)"""
    st, *outs = e.replica_inbox(*S.pack(e.n, msgs))
    return st, (S.decode_outputs(e.n, msgs, outs) if st == 0 else None), outs


def same_as_model(e, model, msgs, state=True):
    st, rows, _ = run(e, msgs)
    want_st, want = model.inbox(msgs)
    assert st == want_st == 0
    for i, (g, w) in enumerate(zip(rows, want)):
        assert g == tuple(w), (i, msgs[i], g, w)
    if state:
        cells, keys = S.touched(msgs, NK)
        assert S.gpu_state(e, cells, keys) == S.model_state(model, cells, keys)


@pytest.mark.parametrize("seed,n,m", MODEL_BURSTS)
def test_against_the_set_model(seed, n, m):
    e, model = ctx(n), IM.InboxModel(n, NK, NI)
    same_as_model(e, model, S.make_burst(seed, n, m))
    # two more bursts on the state the first one left: replies now also answer from entries written before the burst
    same_as_model(e, model, S.make_burst(seed + 100, n, 150, first_triple=3000), state=False)
    same_as_model(e, model, S.make_burst(seed + 200, n, 150, first_triple=6000, max_ordering=5))
    e.close()


def _per_kind(e, msg):
    """one message through the per-kind entry point with target_mask = 1 << to -> the inbox's raw output row
    (outcome, out_ballot, out_status, out_deps, out_values_end, out_triple)"""
    kind, to, L, x, bo, br, key, is_set, tid, w, end = msg
    n = e.n
    one = lambda v: np.asarray([v], np.int32)
    zeros = [0] * n
    stored = lambda: ([int(v) for v in e.read_cmdlog_deps(to, L, x)[0]], e.read_cmdlog_deps(to, L, x)[1], e.read_cmdlog(to, L, x)[3])
    if kind == IM.IN_PRE_ACCEPT:
        st, ok, resend, nack, com, nb, rd, re, rt = e.handle_preaccept(one(L), one(x), one(bo), one(br), one(key), [is_set], one(tid),
                                                                       np.asarray([w], np.int32), one(end), [1 << to])
        assert st == 0
        outcome = (IM.RI_PRE_ACCEPT_OK if ok[0] else IM.RI_PRE_ACCEPT_OK_AGAIN if resend[0] else IM.RI_NACK if nack[0] else
                   IM.RI_COMMIT_BACK if com[0] else IM.RI_IGNORED)
        return (outcome, int(nb[0]) if nack[0] else -1, -1, rd[0, to].tolist(), int(re[0, to]), int(rt[0, to]))
    if kind == IM.IN_COMMIT:
        by_id = w[0] == -1
        assert e.handle_commit(one(L), one(x), one(tid), [1 << to], one(key), [is_set], None if by_id else np.asarray([w], np.int32),
                               None if by_id else one(end)) == 0
        return (IM.RI_LEARNT, -1, -1, zeros, 0, -1)
    assert kind == IM.IN_PREPARE
    st, ok, nack, com, nb, rs, rv, rt = e.prepare(one(L), one(x), one(bo), one(br), [1 << to])
    assert st == 0
    if com[0]:
        d, de, t = stored()
        return (IM.RI_COMMIT_BACK, -1, -1, d, de, t)
    if nack[0]:
        return (IM.RI_NACK, int(nb[0]), -1, zeros, 0, -1)
    if rs[0, to] == 0:
        return (IM.RI_PREPARE_OK, -1, 0, zeros, 0, -1)
    d, de, _ = stored()                                       # (a Prepare leaves the entry's triple as it was)
    return (IM.RI_PREPARE_OK, int(rv[0, to]), int(rs[0, to]), d, de, int(rt[0, to]))


def test_against_the_librarys_own_entry_points():
    n = 5
    msgs = [x for x in S.make_burst(21, n, 260) if x[0] != IM.IN_ACCEPT]    # (an Accept has no single-replica entry point)
    assert len(msgs) >= 150 and {x[0] for x in msgs} == {IM.IN_PRE_ACCEPT, IM.IN_COMMIT, IM.IN_PREPARE}
    a, b = ctx(n), ctx(n)
    st, _, outs = run(a, msgs)
    assert st == 0
    seen = set()
    for i, msg in enumerate(msgs):
        got = (int(outs[0][i]), int(outs[1][i]), int(outs[2][i]), outs[3][i].tolist(), int(outs[4][i]), int(outs[5][i]))
        assert got == _per_kind(b, msg), (i, msg)
        seen.add((msg[0], got[0]))
    assert len(seen) >= 8, seen
    cells, keys = S.touched(msgs, NK)
    assert S.gpu_state(a, cells, keys, raw=True) == S.gpu_state(b, cells, keys, raw=True)
    a.close(), b.close()


def test_a_burst_cut_in_two_is_the_same_burst():
    n = 5
    msgs = S.make_burst(31, n, 600)
    cells, keys = S.touched(msgs, NK)
    whole = ctx(n)
    st, _, want = run(whole, msgs)
    assert st == 0
    rng = random.Random(5)
    for cut in (rng.randrange(1, 599), 1, 599):
        halves = ctx(n)
        st1, _, o1 = run(halves, msgs[:cut])
        st2, _, o2 = run(halves, msgs[cut:])
        assert st1 == st2 == 0
        for w, x, y in zip(want, o1, o2):
            np.testing.assert_array_equal(w, np.concatenate([x, y]))
        assert S.gpu_state(halves, cells[::3], keys, raw=True) == S.gpu_state(whole, cells[::3], keys, raw=True)
        halves.close()
    whole.close()


# a wavefront, a 256-thread block, CL_TILE = 1024, the radix sort's tile of 4096 pairs past one pass of blocks
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257, 1025, 3 * 4096 + 1])
def test_sizes(m):
    n = 5
    e, model = ctx(n), IM.InboxModel(n, NK, NI)
    msgs = S.make_burst(40 + m, n, m)
    assert len(msgs) == m
    st, rows, _ = run(e, msgs)
    want_st, want = model.inbox(msgs)
    assert st == want_st == 0
    if m:
        assert rows == [tuple(w) for w in want]
    cells, keys = S.touched(msgs, NK)
    step = 1 + len(cells) // 200                                  # (a readback is a handful of small copies per cell)
    assert S.gpu_state(e, cells[::step], keys) == S.model_state(model, cells[::step], keys)
    e.close()


def test_one_key_under_every_message():
    n = 5
    e, model = ctx(n), IM.InboxModel(n, NK, NI)
    # every message on key 0 at replica 2: its (replica, key) segment of the scan spans more than four 64-wide chunks
    # (tests/test_epaxos_inbox_cpu.py counts the puts)
    msgs = S.make_burst(3, n, 1025, hot_key=0, hot_to=2)
    st, rows, _ = run(e, msgs)
    assert st == 0 and rows == [tuple(w) for w in model.inbox(msgs)[1]]
    cells, keys = S.touched(msgs, NK)
    assert keys == [0]
    assert S.gpu_state(e, cells[::7], keys) == S.model_state(model, cells[::7], keys)
    e.close()


def test_a_run_of_200_messages_on_one_cell():
    n = 5
    e, model = ctx(n), IM.InboxModel(n, NK, NI)
    same_as_model(e, model, S.make_burst(8, n, 40))               # (something in the log and the index beforehand)
    same_as_model(e, model, S.long_run(n, 200))
    e.close()


def test_einval_leaves_state_and_outputs_untouched():
    n = 5
    e = ctx(n)
    first = S.make_burst(50, n, 120)
    assert run(e, first)[0] == 0
    msgs = S.make_burst(51, n, 90, first_triple=4000)
    cells, keys = S.touched(first + msgs, NK)
    before = S.gpu_state(e, cells, keys, raw=True)
    good = (IM.IN_PRE_ACCEPT, 1, 2, 5, 1, 1, 0, 1, 7, [0, 0, 5, 0, 0], 7)
    bad = []
    for field, value in ((0, 4), (0, -1), (1, n), (1, -1), (2, n), (3, NI), (3, -1), (4, 1 << 27), (4, -1), (5, n), (6, NK),
                         (6, -2), (9, [0, -1, 5, 0, 0]), (9, [0, 0, 4, 0, 0]), (9, [0, 0, 6, 0, 0]), (10, 6)):
        x = list(good)
        x[field] = value
        bad.append(tuple(x))
    bad.append((IM.IN_ACCEPT, 1, 2, 5, 1, n, 0, 1, 7, [-1, 0, 0, 0, 0], 0))                  # an Accept has a ballot
    bad.append((IM.IN_PREPARE, 1, 2, 5, -1, 0, 0, 0, 7, [0] * n, 0))                        # and so has a Prepare
    bad.append((IM.IN_ACCEPT, 1, 2, 5, 1, 1, NK, 1, 7, [-1, 0, 0, 0, 0], 0))                 # an Accept has a command
    bad.append((IM.IN_COMMIT, 1, 2, 5, 0, 0, 0, 1, 7, [0, 0, 6, 0, 0], 7))                   # explicit ids over a cover
    bad.append((IM.IN_COMMIT, 1, 2, 5, 0, 0, 0, 1, 7, [0, 0, 5, 0, 0], 6))                   # explicit ids that are none
    bad.append((IM.IN_ACCEPT, 1, 2, 5, 1, 1, 0, 1, 7, [0, -3, 5, 0, 0], 0))                  # a negative watermark
    model = IM.InboxModel(n, NK, NI)
    for j, x in enumerate(bad):
        assert not model.valid(x), x
        at = (7 * j) % (len(msgs) + 1)
        burst = msgs[:at] + [x] + msgs[at:]
        st, *outs = e.replica_inbox(*S.pack(n, burst))
        assert st == IM.EINVAL, x
        assert all((o == -9).all() for o in outs), x
    assert S.gpu_state(e, cells, keys, raw=True) == before
    # what a Commit and a Prepare do not read may hold anything
    fine = [(IM.IN_COMMIT, 0, 2, 5, -7, 99, 0, 0, 7, [-1, 9, 9, 9, 9], 0), (IM.IN_PREPARE, 0, 2, 6, 0, 0, 99, 0, 7, [0] * n, 0)]
    assert run(e, fine)[0] == 0
    # m above the bound is refused before an array is looked at; a context without a command log has no inbox
    a = S.pack(n, fine)
    p = lambda v: None if v is None else v.ctypes.data
    from frankenpaxos_amd.epaxos import INBOX_MAX, EPaxos
    assert e.L.fpx_epx_replica_inbox(e._h, INBOX_MAX + 1, *[p(v) for v in a], *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox(e._h, -1, *[p(v) for v in a], *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox(e._h, 2, None, *[p(v) for v in a[1:]], *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox(e._h, 2, *[p(v) for v in a], *[None] * 6) == 0          # every output may be NULL
    nolog = EPaxos(n, NK)
    assert nolog.replica_inbox(*a)[0] == IM.EINVAL
    nolog.close(), e.close()


def test_the_device_form_equals_the_host_form():
    import torch

    n = 5
    first, msgs = S.make_burst(60, n, 200), S.make_burst(61, n, 700, first_triple=4000)
    host, dev = ctx(n), ctx(n)
    assert run(host, first)[0] == 0 and run(dev, first)[0] == 0
    a = S.pack(n, msgs)
    want = host.replica_inbox(*a)
    assert want[0] == 0
    m = len(msgs)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(5)]
    odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.replica_inbox_dev(*[T(x) for x in a], outcome=outs[0], out_ballot=outs[1], out_status=outs[2], out_deps=odeps,
                          out_values_end=outs[3], out_triple=outs[4])
    assert dev.sync() == 0
    for got, w in zip([outs[0], outs[1], outs[2], odeps, outs[3], outs[4]], want[1:]):
        assert (got.cpu().numpy() == w).all()
    cells, keys = S.touched(first + msgs, NK)
    assert S.gpu_state(dev, cells, keys, raw=True) == S.gpu_state(host, cells, keys, raw=True)
    # a bad message in the device form: the status comes with sync(), nothing was written
    bad = list(msgs[:50])
    bad[20] = bad[20][:1] + (n,) + bad[20][2:]
    b = S.pack(n, bad)
    mark = torch.full((50,), -9, dtype=torch.int32, device="cuda")
    dev.replica_inbox_dev(*[T(x) for x in b], outcome=mark, out_ballot=mark, out_status=mark, out_values_end=mark, out_triple=mark)
    assert dev.sync() == IM.EINVAL and (mark.cpu().numpy() == -9).all()
    assert S.gpu_state(dev, cells, keys, raw=True) == S.gpu_state(host, cells, keys, raw=True)
    host.close(), dev.close()


def test_the_inbox_ends_leader_states_as_the_reference_does():
    from tests import epaxos_leader_model as M

    n = 5
    e = ctx(n, leader_state=True)
    a32 = lambda v: np.asarray(v, np.int32)
    k = 5                                                         # instances (0, 0 .. 4), led by replica 0 in ballot (0, 0)
    st, deps, dend = e.lead(a32([0] * k), a32(range(k)), a32([0] * k), a32([0] * k), a32([1] * k), [1] * k, a32(range(100, 100 + k)))
    assert st == 0
    assert [e.read_leader_state(0, 0, x)[0][0] for x in range(k)] == [1] * k
    z = [0] * n
    burst = [(IM.IN_PRE_ACCEPT, 0, 0, 0, 1, 1, 1, 1, 200, z, 0),  # a higher-ballot PreAccept (:1239-1242)
             (IM.IN_ACCEPT, 0, 0, 1, 1, 2, 1, 1, 201, [-1] + z[1:], 0),  # ... Accept (:1480-1483)
             (IM.IN_PREPARE, 0, 0, 2, 1, 3, 0, 0, 0, z, 0),       # ... Prepare (:1645-1648)
             (IM.IN_COMMIT, 0, 0, 3, 0, 0, 1, 1, 103, z, 0),      # the instance commits (:831)
             (IM.IN_PRE_ACCEPT, 1, 0, 4, 1, 1, 1, 1, 204, z, 0)]  # another replica's entry: replica 0 goes on leading (0, 4)
    st, rows, _ = run(e, burst)
    assert st == 0
    assert [r[0] for r in rows] == [IM.RI_PRE_ACCEPT_OK, IM.RI_ACCEPT_OK, IM.RI_PREPARE_OK, IM.RI_LEARNT, IM.RI_PRE_ACCEPT_OK]
    assert rows[2][1:3] == (0, 2) and rows[2][4] == 102           # the PrepareOk shows what replica 0 led: PreAccepted, (0, 0)
    assert [e.read_leader_state(0, 0, x)[0][0] for x in range(k)] == [0, 0, 0, 0, 1]
    oks = [(M.PRE_ACCEPT_OK, 0, 0, x, 0, 0, q, 0, deps[x].tolist(), int(dend[x])) for x in range(k) for q in (1, 2, 3)]
    from tests import epaxos_leader_streams as LS
    st, outcome = e.leader_replies(*LS.burst_arrays(n, oks))[:2]
    assert st == 0
    assert outcome[:12].tolist() == [M.IGNORED] * 12              # the replies of the four ended states are ignored
    assert M.IGNORED not in outcome[12:].tolist() and M.FAST_COMMIT in outcome[12:].tolist()
    e.close()


def test_a_repeated_instance_is_refused_by_the_per_kind_call_and_handled_by_the_inbox():
    n = 5
    z = [0] * n
    burst = [(IM.IN_PRE_ACCEPT, 2, 0, 7, 0, 0, 1, 1, 300, z, 0), (IM.IN_PRE_ACCEPT, 2, 1, 3, 0, 1, 1, 0, 301, z, 0),
             (IM.IN_PRE_ACCEPT, 2, 0, 7, 0, 0, 1, 1, 300, z, 0)]  # the leader's PreAccept of (0, 7), sent again
    cols = [np.asarray(c, np.int32) for c in zip(*[x[:9] for x in burst])]
    old, new = ctx(n), ctx(n)
    res = old.handle_preaccept(cols[2], cols[3], cols[4], cols[5], cols[6], cols[7].astype(np.uint8), cols[8],
                               np.zeros((3, n), np.int32), np.zeros(3, np.int32), [1 << 2] * 3)
    assert res[0] == IM.EINVAL
    st, rows, _ = run(new, burst)
    assert st == 0 and [r[0] for r in rows] == [IM.RI_PRE_ACCEPT_OK, IM.RI_PRE_ACCEPT_OK, IM.RI_PRE_ACCEPT_OK_AGAIN]
    # (the get of (1, 3) conflicts with the set of (0, 7): a top-one index answers with the prefix up to it)
    assert rows[2][3:] == rows[0][3:] == (frozenset(), 300) and rows[1][3] == frozenset((0, y) for y in range(8))
    model = IM.InboxModel(n, NK, NI)
    assert [tuple(w) for w in model.inbox(burst)[1]] == rows
    old.close(), new.close()


def test_one_burst_through_the_native(jvm):  # noqa: F811
    n = 5
    msgs = S.make_burst(70, n, 300)
    a = S.pack(n, msgs)
    m = len(msgs)
    ref = ctx(n)
    want = ref.replica_inbox(*a)
    assert want[0] == 0
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    i32 = lambda v: jvm.arr(np.asarray(v, np.int32).reshape(-1))
    ins = [i32(v) for v in a[:7]] + [jvm.arr(a[7].astype(np.int8))] + [i32(a[8]), i32(a[9]), i32(a[10])]
    outcome, reply, odeps = jvm.arr(np.full(m, -9, np.int32)), jvm.arr(np.full(4 * m, -9, np.int32)), jvm.arr(np.full(m * n, -9, np.int32))
    # every array is length-checked before native code touches it; the handle is the authority on n
    for j in range(11):
        short = list(ins)
        short[j] = jvm.arr(np.zeros(len(a[j].reshape(-1)) - 1, np.int8 if j == 7 else np.int32))
        assert jvm.call("epxReplicaInbox", C.c_int32, h, m, n, *short, outcome, reply, odeps) == 1
    assert jvm.call("epxReplicaInbox", C.c_int32, h, m, n, *ins, outcome, jvm.arr(np.zeros(4 * m - 1, np.int32)), odeps) == 1
    assert jvm.call("epxReplicaInbox", C.c_int32, h, m, 3, *ins, outcome, reply, odeps) == 1
    assert (jvm.read(outcome, np.int32, m) == -9).all()
    assert jvm.call("epxReplicaInbox", C.c_int32, h, m, n, *ins, outcome, reply, odeps) == 0
    np.testing.assert_array_equal(jvm.read(outcome, np.int32, m), want[1])
    r = jvm.read(reply, np.int32, 4 * m).reshape(4, m)
    for got, w in zip(r, (want[2], want[3], want[5], want[6])):
        np.testing.assert_array_equal(got, w)
    np.testing.assert_array_equal(jvm.read(odeps, np.int32, m * n).reshape(m, n), want[4])
    assert jvm.call("epxReplicaInbox", C.c_int32, h, 0, n, *[None] * 14) == 0                # an empty burst
    assert jvm.call("epxDestroy", C.c_int32, h) == 0
    ref.close()
