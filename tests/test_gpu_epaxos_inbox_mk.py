"""fpx_epx_replica_inbox_mk[_dev]: a burst of PreAccept / Accept / Commit / Prepare messages whose commands carry KEY LISTS,
in one device call: against tests/epaxos_inbox_mk_model.py (the multi-key set model, one message at a time) on every output
and on the command log, largestBallot and every key's index rows; against fpx_epx_replica_inbox bit for bit on one-key
lists; against the library's own per-kind _mk entry points; against itself with the burst cut in two; at the sizes where the
kernels take another path.  tests/test_epaxos_inbox_mk_cpu.py asserts what the generated bursts exercise."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_mk_model as MM
from tests import epaxos_inbox_mk_streams as MS
from tests import epaxos_inbox_streams as S
from tests.test_epaxos_inbox_mk_cpu import MODEL_BURSTS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock-JVM fixture)

pytestmark = pytest.mark.gpu
NK, NI = 4, 64


def ctx(n, num_keys=NK, num_instances=NI, leader_state=False):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, num_keys, num_instances=num_instances, leader_state=leader_state)


def run(e, msgs):
    """(status, the outputs decoded into the model's rows, the raw output arrays)"""
    st, *outs = e.replica_inbox_mk(*MS.pack(e.n, msgs))
    return st, (S.decode_outputs(e.n, msgs, outs) if st == 0 else None), outs


def state(e, msgs, step=1, raw=False, num_keys=NK):
    return S.gpu_state(e, MS.cells_of(msgs)[::step], MS.all_keys(num_keys), raw=raw)


def same_as_model(e, model, msgs, step=1, num_keys=NK):
    st, rows, _ = run(e, msgs)
    want_st, want = model.inbox(msgs)
    assert st == want_st == 0
    for i, (g, w) in enumerate(zip(rows, want)):
        assert g == tuple(w), (i, msgs[i], g, w)
    cells = MS.cells_of(msgs)[::step]
    assert S.gpu_state(e, cells, MS.all_keys(num_keys)) == S.model_state(model, cells, MS.all_keys(num_keys))


@pytest.mark.parametrize("seed,n,m", MODEL_BURSTS)
def test_against_the_set_model(seed, n, m):
    e, model = ctx(n), MM.InboxMkModel(n, NK, NI)
    step = 1 + m // 300
    same_as_model(e, model, MS.make_burst(seed, n, m), step)
    # a second burst on the state the first one left: it meets the first's entries and index
    same_as_model(e, model, MS.make_burst(seed + 100, n, min(m, 150), first_triple=3000, max_ordering=5))
    e.close()


def test_one_key_lists_equal_the_single_key_call_bit_for_bit():
    import torch

    n = 5
    a, b, d = ctx(n), ctx(n), ctx(n)                          # the single-key call, the host form, the device form
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for seed, m, first in ((81, 700, 1000), (82, 300, 5000)):
        lists = MS.make_burst(seed, n, m, one_key=True, first_triple=first)
        # every eighth script a Noop: the empty list on one side, key -1 on the other
        lists = [x[:6] + ((),) + x[7:] if (x[2] + x[3]) % 8 == 0 else x for x in lists]
        single = MS.single_key_form(lists)
        want = a.replica_inbox(*S.pack(n, single))
        got = b.replica_inbox_mk(*MS.pack(n, lists))
        assert want[0] == got[0] == 0
        for w, g in zip(want[1:], got[1:]):
            np.testing.assert_array_equal(w, g)
        p = MS.pack(n, lists)
        outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(5)]
        odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
        off, keys = p[6]
        d.replica_inbox_mk_dev(*[T(x) for x in p[:6]], T(off), T(keys), *[T(x) for x in p[7:]], outcome=outs[0],
                               out_ballot=outs[1], out_status=outs[2], out_deps=odeps, out_values_end=outs[3], out_triple=outs[4])
        assert d.sync() == 0
        for w, g in zip(want[1:], [outs[0], outs[1], outs[2], odeps, outs[3], outs[4]]):
            np.testing.assert_array_equal(w, g.cpu().numpy())
    # over ALL cells and keys of the context
    cells = [(r, (L, x)) for r in range(n) for L in range(n) for x in range(NI)]
    want = S.gpu_state(a, cells, MS.all_keys(NK), raw=True)
    assert S.gpu_state(b, cells, MS.all_keys(NK), raw=True) == want
    assert S.gpu_state(d, cells, MS.all_keys(NK), raw=True) == want
    a.close(), b.close(), d.close()


def _per_kind(e, msg):
    """one message through the per-kind _mk entry point with target_mask = 1 << to -> the inbox's raw output row"""
    kind, to, L, x, bo, br, keys, is_set, tid, w, end = msg
    n = e.n
    one = lambda v: np.asarray([v], np.int32)
    zeros = [0] * n
    stored = lambda: ([int(v) for v in e.read_cmdlog_deps(to, L, x)[0]], e.read_cmdlog_deps(to, L, x)[1], e.read_cmdlog(to, L, x)[3])
    if kind == IM.IN_PRE_ACCEPT:
        st, ok, resend, nack, com, nb, rd, re, rt = e.handle_preaccept_mk(one(L), one(x), one(bo), one(br), [list(keys)], [is_set],
                                                                          one(tid), np.asarray([w], np.int32), one(end), [1 << to])
        assert st == 0
        outcome = (IM.RI_PRE_ACCEPT_OK if ok[0] else IM.RI_PRE_ACCEPT_OK_AGAIN if resend[0] else IM.RI_NACK if nack[0] else
                   IM.RI_COMMIT_BACK if com[0] else IM.RI_IGNORED)
        return (outcome, int(nb[0]) if nack[0] else -1, -1, rd[0, to].tolist(), int(re[0, to]), int(rt[0, to]))
    if kind == IM.IN_COMMIT:
        by_id = w[0] == -1
        assert e.handle_commit_mk(one(L), one(x), one(tid), [1 << to], [list(keys)], [is_set],
                                  None if by_id else np.asarray([w], np.int32), None if by_id else one(end)) == 0
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
    d, de, _ = stored()
    return (IM.RI_PREPARE_OK, int(rv[0, to]), int(rs[0, to]), d, de, int(rt[0, to]))


def test_against_the_librarys_own_mk_entry_points():
    n = 5
    # instances pairwise distinct (what those calls require), no Accept (it has no single-replica entry point); a first
    # burst leaves entries for the second to be answered from
    a, b = ctx(n), ctx(n)
    seen = set()
    for seed, first, top in ((21, 1000, 3), (22, 4000, 3), (23, 7000, 0)):   # (the last one: ballots that fall behind)
        msgs = MS.distinct_instances([x for x in MS.make_burst(seed, n, 400, first_triple=first, max_ordering=top)
                                      if x[0] != IM.IN_ACCEPT])
        assert len(msgs) >= 60 and {x[0] for x in msgs} == {IM.IN_PRE_ACCEPT, IM.IN_COMMIT, IM.IN_PREPARE}
        st, _, outs = run(a, msgs)
        assert st == 0
        for i, msg in enumerate(msgs):
            got = (int(outs[0][i]), int(outs[1][i]), int(outs[2][i]), outs[3][i].tolist(), int(outs[4][i]), int(outs[5][i]))
            assert got == _per_kind(b, msg), (i, msg)
            seen.add((msg[0], got[0]))
        assert state(a, msgs, raw=True) == state(b, msgs, raw=True)
    # processed, Nack and the Commit back for a PreAccept and for a Prepare, and a Commit learnt
    assert seen == {(0, IM.RI_PRE_ACCEPT_OK), (0, IM.RI_NACK), (0, IM.RI_COMMIT_BACK), (2, IM.RI_LEARNT), (3, IM.RI_PREPARE_OK),
                    (3, IM.RI_NACK), (3, IM.RI_COMMIT_BACK)}, seen
    a.close(), b.close()


def test_a_burst_cut_in_two_is_the_same_burst():
    n = 5
    msgs = MS.make_burst(31, n, 600)
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
        assert state(halves, msgs, 3, raw=True) == state(whole, msgs, 3, raw=True)
        halves.close()
    whole.close()


# a wavefront, a 256-thread block, CL_TILE = 1024, the radix sort's tile of 4096 pairs past one pass of blocks
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257, 1025, 3 * 4096 + 1])
def test_sizes(m):
    n = 5
    e, model = ctx(n), MM.InboxMkModel(n, NK, NI)
    msgs = MS.make_burst(40 + m, n, m)
    assert len(msgs) == m
    st, rows, _ = run(e, msgs)
    want_st, want = model.inbox(msgs)
    assert st == want_st == 0
    if m:
        assert rows == [tuple(w) for w in want]
    cells = MS.cells_of(msgs)
    cells = cells[::1 + len(cells) // 200]
    assert S.gpu_state(e, cells, MS.all_keys(NK)) == S.model_state(model, cells, MS.all_keys(NK))
    e.close()


# the pair count exactly at a scan-tile boundary, and no pairs at all under m > 0 messages
@pytest.mark.parametrize("pairs", [0, 1023, 1024, 1025])
def test_pair_counts(pairs):
    n = 5
    e, model = ctx(n), MM.InboxMkModel(n, NK, NI)
    msgs = MS.make_burst(90 + pairs, n, 300)
    assert pairs == 0 or sum(len(x[6]) for x in msgs) < 1000      # (the last command's list is padded up to the count)
    msgs = MS.with_pairs(msgs, pairs)
    assert sum(len(x[6]) for x in msgs) == pairs and len(msgs) == 300
    same_as_model(e, model, msgs, 2)
    same_as_model(e, model, MS.make_burst(95, n, 60, first_triple=7000))      # (and the context is fit for the next burst)
    e.close()


def test_one_command_of_300_keys():
    n, nk = 5, 512
    e, model = ctx(n, num_keys=nk), MM.InboxMkModel(n, nk, NI)
    rng = random.Random(300)
    long_list = tuple(rng.randrange(nk) for _ in range(300))
    assert 150 < len(set(long_list)) < 300                       # repeats inside it: the quadratic distinct-key check
    z = [0] * n
    small = lambda k: tuple(long_list[(7 * k + j) % 300] for j in range(3))
    msgs = [(IM.IN_COMMIT, 2, 1, k, 0, 0, small(k), k & 1, 100 + k, z, 0) for k in range(20)]
    msgs.append((IM.IN_PRE_ACCEPT, 2, 0, 9, 0, 0, long_list, 1, 200, z, 0))              # its pairs run across scan tiles
    msgs += [(IM.IN_PRE_ACCEPT, 2, 3, k, 0, 3, small(k + 40), 0, 300 + k, z, 0) for k in range(20)]
    msgs.append((IM.IN_PRE_ACCEPT, 2, 4, 5, 1, 4, long_list[::-1], 0, 400, z, 0))
    st, rows, _ = run(e, msgs)
    want_st, want = model.inbox(msgs)
    assert st == want_st == 0 and rows == [tuple(w) for w in want]
    assert rows[20][3] and rows[-1][3]                            # both long commands found conflicts
    keys = sorted(set(long_list))[::5]
    cells = MS.cells_of(msgs)
    assert S.gpu_state(e, cells, keys) == S.model_state(model, cells, keys)
    e.close()


def test_a_hot_key_in_every_list():
    n = 5
    e, model = ctx(n), MM.InboxMkModel(n, NK, NI)
    # key 0 in every command, all messages to replica 2: its (replica, key) segment of the scan is one long run
    msgs = MS.make_burst(3, n, 1025, hot_key=0, hot_to=2)
    assert all(0 in x[6] for x in msgs) and {x[1] for x in msgs} == {2}
    same_as_model(e, model, msgs, 7)
    e.close()


def test_einval_leaves_state_and_outputs_untouched():
    import torch

    n = 5
    e = ctx(n)
    first = MS.make_burst(50, n, 120)
    assert run(e, first)[0] == 0
    msgs = MS.make_burst(51, n, 90, first_triple=4000)
    before = state(e, first + msgs, raw=True)
    p = MS.pack(n, msgs)
    off, keys = p[6]
    assert len(keys) > 20

    def refused(off2, keys2):
        q = list(p)
        q[6] = (np.asarray(off2, np.int32), np.asarray(keys2, np.int32))
        st, *outs = e.replica_inbox_mk(*q)
        assert st == IM.EINVAL
        assert all((o == -9).all() for o in outs)

    # the host form: the list rules
    bad = off.copy(); bad[30], bad[31] = off[31] + 1, off[30]     # not monotone
    refused(bad, keys)
    refused(off + 1, np.concatenate([keys, [0]]))                 # key_offsets[0] = 1
    for value in (NK, -1):
        k2 = keys.copy(); k2[len(keys) // 2] = value
        refused(off, k2)
    # ... and today's message-level errors, each once, with valid lists
    good = (IM.IN_PRE_ACCEPT, 1, 2, 5, 1, 1, (0, 3, 0), 1, 7, [0, 0, 5, 0, 0], 7)
    model = MM.InboxMkModel(n, NK, NI)
    assert model.valid(good)
    wrong = []
    for field, value in ((0, 4), (0, -1), (1, n), (1, -1), (2, n), (3, NI), (3, -1), (4, 1 << 27), (4, -1), (5, n),
                         (9, [0, -1, 5, 0, 0]), (9, [0, 0, 4, 0, 0]), (9, [0, 0, 6, 0, 0]), (10, 6)):
        x = list(good)
        x[field] = value
        wrong.append(tuple(x))
    wrong.append((IM.IN_ACCEPT, 1, 2, 5, 1, n, (0, 1), 1, 7, [-1, 0, 0, 0, 0], 0))
    wrong.append((IM.IN_PREPARE, 1, 2, 5, -1, 0, (), 0, 7, [0] * n, 0))
    wrong.append((IM.IN_COMMIT, 1, 2, 5, 0, 0, (2,), 1, 7, [0, 0, 6, 0, 0], 7))
    wrong.append((IM.IN_COMMIT, 1, 2, 5, 0, 0, (2, 2), 1, 7, [0, 0, 5, 0, 0], 6))
    wrong.append((IM.IN_ACCEPT, 1, 2, 5, 1, 1, (1,), 1, 7, [0, -3, 5, 0, 0], 0))
    for j, x in enumerate(wrong):
        assert not model.valid(x), x
        at = (7 * j) % (len(msgs) + 1)
        st, *outs = e.replica_inbox_mk(*MS.pack(n, msgs[:at] + [x] + msgs[at:]))
        assert st == IM.EINVAL, x
        assert all((o == -9).all() for o in outs), x
    assert state(e, first + msgs, raw=True) == before
    # the device form: num_pairs is not key_offsets[m]; the lists are checked on the device
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    m = len(msgs)
    dev = [T(x) for x in p[:6]] + [T(off), T(np.concatenate([keys, [0, 0]]))] + [T(x) for x in p[7:]]
    for num_pairs, off2 in ((len(keys) + 1, off), (len(keys) - 1, off), (len(keys), bad), (len(keys), off + 1)):
        mark = torch.full((m,), -9, dtype=torch.int32, device="cuda")
        marks = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
        args = list(dev)
        args[6] = T(off2)
        e.replica_inbox_mk_dev(*args, outcome=mark, out_ballot=mark, out_status=mark, out_deps=marks, out_values_end=mark,
                               out_triple=mark, num_pairs=num_pairs)
        assert e.sync() == IM.EINVAL, num_pairs
        assert (mark.cpu().numpy() == -9).all() and (marks.cpu().numpy() == -9).all()
    assert state(e, first + msgs, raw=True) == before
    # bounds that are refused before an array is looked at
    from frankenpaxos_amd.epaxos import INBOX_MAX
    ptr = [None if v is None else v.ctypes.data for v in p[:6] + [off, keys] + p[7:]]
    assert e.L.fpx_epx_replica_inbox_mk(e._h, INBOX_MAX + 1, *ptr, *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox_mk(e._h, m, *ptr[:6], None, *ptr[7:], *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox_mk_dev(e._h, m, *[t.data_ptr() for t in dev[:8]], MM.MAX_PAIRS + 1,
                                            *[t.data_ptr() for t in dev[8:]], *[None] * 6) == IM.EINVAL
    assert e.L.fpx_epx_replica_inbox_mk(e._h, m, *ptr, *[None] * 6) == 0                    # every output may be NULL
    e.close()


def test_the_device_form_equals_the_host_form():
    import torch

    n = 5
    first, msgs = MS.make_burst(60, n, 200), MS.make_burst(61, n, 700, first_triple=4000)
    host, dev = ctx(n), ctx(n)
    assert run(host, first)[0] == 0 and run(dev, first)[0] == 0
    p = MS.pack(n, msgs)
    want = host.replica_inbox_mk(*p)
    assert want[0] == 0
    m = len(msgs)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(5)]
    odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
    off, keys = p[6]
    dev.replica_inbox_mk_dev(*[T(x) for x in p[:6]], T(off), T(keys), *[T(x) for x in p[7:]], outcome=outs[0], out_ballot=outs[1],
                             out_status=outs[2], out_deps=odeps, out_values_end=outs[3], out_triple=outs[4])
    assert dev.sync() == 0
    for got, w in zip([outs[0], outs[1], outs[2], odeps, outs[3], outs[4]], want[1:]):
        assert (got.cpu().numpy() == w).all()
    assert state(dev, first + msgs, raw=True) == state(host, first + msgs, raw=True)
    host.close(), dev.close()


def test_the_inbox_ends_leader_states_as_the_reference_does():
    from frankenpaxos_amd.epaxos import KEY_LIST
    from tests import epaxos_leader_model as M
    from tests import epaxos_leader_streams as LS

    n = 5
    e = ctx(n, leader_state=True)
    a32 = lambda v: np.asarray(v, np.int32)
    k = 5                                                         # instances (0, 0 .. 4), led by replica 0 in ballot (0, 0)
    st, deps, dend = e.lead_mk(a32([0] * k), a32(range(k)), a32([0] * k), a32([0] * k), [[1, 2]] * k, [1] * k, a32(range(100, 100 + k)))
    assert st == 0
    assert [e.read_leader_state(0, 0, x)[0][0] for x in range(k)] == [1] * k
    assert [e.read_leader_state(0, 0, x)[0][4] for x in range(k)] == [KEY_LIST] * k
    z = [0] * n
    burst = [(IM.IN_PRE_ACCEPT, 0, 0, 0, 1, 1, (1, 2), 1, 200, z, 0),    # a higher-ballot PreAccept (:1239-1242)
             (IM.IN_ACCEPT, 0, 0, 1, 1, 2, (1, 2), 1, 201, [-1] + z[1:], 0),    # ... Accept (:1480-1483)
             (IM.IN_PREPARE, 0, 0, 2, 1, 3, (), 0, 0, z, 0),             # ... Prepare (:1645-1648)
             (IM.IN_COMMIT, 0, 0, 3, 0, 0, (1, 2), 1, 103, z, 0),        # the instance commits (:831)
             (IM.IN_PRE_ACCEPT, 1, 0, 4, 1, 1, (1, 2), 1, 204, z, 0)]    # another replica's entry: replica 0 goes on leading (0, 4)
    st, rows, _ = run(e, burst)
    assert st == 0
    assert [r[0] for r in rows] == [IM.RI_PRE_ACCEPT_OK, IM.RI_ACCEPT_OK, IM.RI_PREPARE_OK, IM.RI_LEARNT, IM.RI_PRE_ACCEPT_OK]
    assert rows[2][1:3] == (0, 2) and rows[2][4] == 102
    assert [e.read_leader_state(0, 0, x)[0][0] for x in range(k)] == [0, 0, 0, 0, 1]
    oks = [(M.PRE_ACCEPT_OK, 0, 0, x, 0, 0, q, 0, deps[x].tolist(), int(dend[x])) for x in range(k) for q in (1, 2, 3)]
    st, outcome = e.leader_replies(*LS.burst_arrays(n, oks))[:2]
    assert st == 0
    assert outcome[:12].tolist() == [M.IGNORED] * 12
    assert M.IGNORED not in outcome[12:].tolist() and M.FAST_COMMIT in outcome[12:].tolist()
    e.close()


def test_one_burst_through_the_native(jvm):  # noqa: F811
    n = 5
    msgs = MS.make_burst(70, n, 300)
    p = MS.pack(n, msgs)
    off, keys = p[6]
    a = p[:6] + [off, keys] + p[7:]
    m = len(msgs)
    ref = ctx(n)
    want = ref.replica_inbox_mk(*p)
    assert want[0] == 0
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    i32 = lambda v: jvm.arr(np.asarray(v, np.int32).reshape(-1))
    ins = [i32(v) for v in a[:8]] + [jvm.arr(a[8].astype(np.int8))] + [i32(a[9]), i32(a[10]), i32(a[11])]
    outcome, reply, odeps = jvm.arr(np.full(m, -9, np.int32)), jvm.arr(np.full(4 * m, -9, np.int32)), jvm.arr(np.full(m * n, -9, np.int32))
    # every array is length-checked before native code touches it; the handle is the authority on n
    for j in range(12):
        short = list(ins)
        short[j] = jvm.arr(np.zeros(len(a[j].reshape(-1)) - 1, np.int8 if j == 8 else np.int32))
        assert jvm.call("epxReplicaInboxMk", C.c_int32, h, m, n, *short, outcome, reply, odeps) == 1, j
    assert jvm.call("epxReplicaInboxMk", C.c_int32, h, m, n, *ins, outcome, jvm.arr(np.zeros(4 * m - 1, np.int32)), odeps) == 1
    assert jvm.call("epxReplicaInboxMk", C.c_int32, h, m, 3, *ins, outcome, reply, odeps) == 1
    assert (jvm.read(outcome, np.int32, m) == -9).all()
    assert jvm.call("epxReplicaInboxMk", C.c_int32, h, m, n, *ins, outcome, reply, odeps) == 0
    np.testing.assert_array_equal(jvm.read(outcome, np.int32, m), want[1])
    r = jvm.read(reply, np.int32, 4 * m).reshape(4, m)
    for got, w in zip(r, (want[2], want[3], want[5], want[6])):
        np.testing.assert_array_equal(got, w)
    np.testing.assert_array_equal(jvm.read(odeps, np.int32, m * n).reshape(m, n), want[4])
    assert jvm.call("epxReplicaInboxMk", C.c_int32, h, 0, n, *[None] * 15) == 0              # an empty burst
    assert jvm.call("epxDestroy", C.c_int32, h) == 0
    ref.close()
