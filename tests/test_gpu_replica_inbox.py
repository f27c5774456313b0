"""fpx_replica_inbox / _dev (include/fpx.h): a burst of a MultiPaxos replica's inbox, Chosens and reads interleaved,
scheduled in one device call -- against the message-at-a-time model of tests/replica_inbox_model.py (shaped like
multipaxos/Replica.scala): exec_count, reply_slot, order, counts, (executed_watermark, num_chosen) and the whole log,
equal, for the host form and the _dev form.  The pinned cases spell their expectation out by hand.  The streams are
tests/replica_inbox_streams.py; tests/test_replica_inbox_cpu.py holds that they reach every class of read.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import replica_inbox_model as M
from tests import replica_inbox_streams as RS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL = 1
S0 = 4096
CH, RD, SEQ, EV = wire.CHOSEN, wire.READ_REQUEST, wire.SEQUENTIAL_READ_REQUEST, wire.EVENTUAL_READ_REQUEST
RDB, SEQB, EVB = wire.READ_REQUEST_BATCH, wire.SEQUENTIAL_READ_REQUEST_BATCH, wire.EVENTUAL_READ_REQUEST_BATCH
# the executed-by scan (csrc/fpx_replica_inbox.hpp): a tile is RI_TILE slots, k_ri_tilescan takes RI_SCAN_THREADS tiles a step
RI_TILE, RI_SCAN_THREADS = 256, 1024


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def context(fa, S=S0, **more):
    return fa.Context(fa.make_config(**dict(dict(num_slots=S, num_replicas=3, f=1), **more)))


def state_of(gpu):
    vals, pres = gpu.replica_read_log(0, gpu.S)
    return (pres, vals) + gpu.replica_state()


def call(gpu, kind, slot, value, mask=None, dev=False):
    """one burst on the GPU as a model Result (the log is read back)"""
    kind, slot, value = (np.ascontiguousarray(a, np.int32) for a in (kind, slot, value))
    n = len(kind)
    if dev:
        import torch

        d = [torch.from_numpy(a).cuda() for a in (kind, slot, value)]
        dm = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
        outs = [torch.full((max(n, 1),), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
        counts = torch.full((4,), -9, dtype=torch.int32, device="cuda")
        gpu.replica_inbox_dev(*d, dm, *outs, counts, n=n)
        st = gpu.sync()
        ec, rs, od = (o.cpu().numpy()[:n] for o in outs)
        counts = counts.cpu().numpy()
        wm, nc = gpu.replica_state()
    else:
        st, ec, rs, od, counts, wm, nc = gpu.replica_inbox(kind, slot, value, mask)
        assert (wm, nc) == gpu.replica_state()
    if st:
        return M.Result(status=st, bad_index=gpu.error_detail()[0]), (ec, rs, od, counts)
    vals, pres = gpu.replica_read_log(0, gpu.S)
    assert wm == counts[3]
    return M.Result(0, -1, ec, rs, od[:counts[0]], tuple(int(c) for c in counts), nc, pres, vals), None


def run(gpu, kind, slot, value, mask=None, dev=False):
    """one burst on the GPU and in the message-at-a-time model, from the GPU's state: equal; returns the result"""
    want = M.sequential(*state_of(gpu), kind, slot, value, mask)
    assert want.status == 0
    got, _ = call(gpu, kind, slot, value, mask, dev)
    M.assert_same(got, want)
    return got


def burst_of(msgs):
    """[(kind, slot, value[, mask])] -> arrays"""
    k, s, v = (np.array([m[j] for m in msgs], np.int32) for j in range(3))
    return k, s, v, np.array([m[3] if len(m) > 3 else 1 for m in msgs], np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# pinned cases: one per class of tests/replica_inbox_model.py CLASSES, expectations by hand
# ---------------------------------------------------------------------------------------------------------------------
PINNED = [
    # W0 = 3 after the first burst (slots 0 1 2), slot 6 in the log above the watermark
    (CH, 0, 10), (CH, 1, 11), (CH, 2, 12), (CH, 6, 16),
]
BURST = [
    (RD, 1, 0),          # 0  r < W0: at once, 3 entries executed, reply slot 2
    (RD, -1, 0),         # 1  r = -1 (a read batcher's): at once
    (EV, 77, 0),         # 2  eventual: at once whatever its slot field says
    (RD, 4, 0),          # 3  deferred under 4
    (SEQ, 4, 0),         # 4  deferred under 4 too: two reads under one slot
    (RDB, 6, 0),         # 5  a batch under slot 6, which is in the log above the watermark: deferred
    (CH, 3, 13),         # 6  executes 3 alone
    (RD, 3, 0),          # 7  at once because of message 6: 4 entries executed, reply slot 3
    (CH, 5, 15),         # 8  a hole at 4: nothing executes
    (CH, 5, 99),         # 9  a duplicate Chosen: ignored
    (EVB, 0, 0, 0),      # 10 masked out: not a read
    (CH, 4, 14),         # 11 fills the hole: 4 5 6 execute at once; 3 and 4 are released after slot 4 with reply slot 3 (r - 1),
                         #    5 after slot 6 with reply slot 5
    (SEQB, 8, 0),        # 12 still deferred, r < num_slots
    (RD, S0, 0),         # 13 still deferred, r >= num_slots
    (RD, 2**31 - 1, 0),  # 14 still deferred
    (EVB, -1, 0),        # 15 eventual batch at the end: 7 entries executed, reply slot 6
    (wire.PHASE2A, 2, 0),  # 16 another kind
]
WANT_EXEC = [3, 3, 3, 5, 5, 7, -2, 4, -2, -2, -2, -2, -1, -1, -1, 7, -2]
WANT_REPLY = [2, 2, 2, 3, 3, 5, -2, 3, -2, -2, -2, -2, -1, -1, -1, 6, -2]
WANT_ORDER = [0, 1, 2, 7, 3, 4, 5, 15, 12, 13, 14]


@pytest.mark.parametrize("dev", [False, True])
def test_pinned_cases(fa, dev):
    gpu = context(fa)
    first = run(gpu, *burst_of(PINNED), dev=dev)
    assert first.counts == (0, 0, 0, 3) and first.num_chosen == 4
    got = run(gpu, *burst_of(BURST), dev=dev)
    assert got.exec_count.tolist() == WANT_EXEC and got.reply_slot.tolist() == WANT_REPLY
    assert got.order.tolist() == WANT_ORDER and got.counts == (11, 8, 3, 7) and got.num_chosen == 7
    assert got.values[:8].tolist() == [10, 11, 12, 13, 14, 15, 16, -1]
    # the hand-back: the still-deferred reads at the front of the next burst, then Chosens 7 and 8
    left = [BURST[i] for i in got.still_deferred()]
    nxt = run(gpu, *burst_of(left + [(CH, 8, 18), (RD, 8, 0), (CH, 7, 17)]), dev=dev)
    assert nxt.exec_count.tolist() == [9, -1, -1, -2, 9, -2] and nxt.reply_slot.tolist() == [7, -1, -1, -2, 7, -2]
    assert nxt.order.tolist() == [0, 4, 1, 2] and nxt.counts == (4, 2, 7, 9)
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# seeded streams
# ---------------------------------------------------------------------------------------------------------------------
def primed(fa, b):
    gpu = context(fa, b.num_slots)
    st, wm, nc = gpu.replica_chosen(b.init_slot, b.init_value)
    assert (st, wm, nc) == (0, b.w0, len(b.init_slot))
    return gpu


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", RS.SIZES)
def test_seeded_streams_equal_the_model(fa, n, dev):
    for seed in RS.SEEDS:
        b = RS.make(seed, n)
        gpu = primed(fa, b)
        got = run(gpu, *b.arrays(), dev=dev)
        if n >= 255:
            assert got.counts[1] > 20 and got.counts[0] - got.counts[1] > 10 and got.counts[3] > got.counts[2] + 50
        if seed == 1:
            run(gpu, b.kind, b.slot, b.value, None, dev=dev)        # the same again without a mask: every Chosen is a duplicate
        gpu.close()


@pytest.mark.parametrize("dev", [False, True])
def test_two_bursts_equal_one(fa, dev):
    for n, k in ((257, 100), (3000, 1234)):
        b = RS.make(2, n)
        one, two = primed(fa, b), primed(fa, b)
        whole = run(one, *b.arrays(), dev=dev)
        head = run(two, *(a[:k] for a in b.arrays()), dev=dev)
        assert len(head.still_deferred()) >= 3                 # the hand-back is not empty
        (kind, slot, value, mask), idx = RS.resubmit(b, k, head.still_deferred())
        tail = run(two, kind, slot, value, mask, dev=dev)
        exec_count, reply_slot = whole.exec_count.copy(), whole.reply_slot.copy()
        exec_count[:k], reply_slot[:k] = head.exec_count, head.reply_slot
        again = tail.exec_count != M.NOT_A_READ
        exec_count[idx[again]], reply_slot[idx[again]] = tail.exec_count[again], tail.reply_slot[again]
        np.testing.assert_array_equal(exec_count, whole.exec_count)
        np.testing.assert_array_equal(reply_slot, whole.reply_slot)
        ran = np.concatenate([head.order[:head.counts[1]], idx[tail.order[:tail.counts[1]]]])
        np.testing.assert_array_equal(ran, whole.order[:whole.counts[1]])
        np.testing.assert_array_equal(idx[tail.still_deferred()], whole.still_deferred())
        assert state_of(one)[2:] == state_of(two)[2:]
        np.testing.assert_array_equal(state_of(one)[1], state_of(two)[1])
        one.close(), two.close()


def test_the_executed_span_crosses_the_second_level_of_the_scan(fa):
    """[W0, W1) longer than RI_TILE * RI_SCAN_THREADS slots: k_ri_tilescan takes a second step and carries the maximum"""
    span = RI_TILE * RI_SCAN_THREADS + 3 * RI_TILE + 57
    S = span + 512
    assert S <= 1 << 21
    rng = np.random.default_rng(11)
    w0 = 100
    gpu = context(fa, S)
    assert gpu.replica_chosen(np.arange(w0), np.arange(w0))[:2] == (0, w0)
    # the Chosens of w0 .. w0 + span - 1 in blocks of 5000 slots, each block shuffled; slot w0 + 7 comes last of all (everything
    # executes in its executeLog, with executed-by = its index: the maximum carried across every tile) -- except the tail
    # from `late` on, which comes after it block by block
    slots = np.arange(w0, w0 + span)
    for lo in range(0, span, 5000):
        rng.shuffle(slots[lo:lo + 5000])
    late = span - 2 * 5000
    order = np.concatenate([slots[:late][slots[:late] != w0 + 7], [w0 + 7], slots[late:]])
    nreads = 4000
    at = np.sort(rng.integers(0, len(order), nreads))
    kind = np.full(len(order) + nreads, CH, np.int32)
    slot = np.zeros(len(order) + nreads, np.int32)
    pos = at + np.arange(nreads)
    kind[pos] = np.array([RD, SEQ, RDB, EV], np.int32)[rng.integers(0, 4, nreads)]
    is_read = np.zeros(len(kind), bool)
    is_read[pos] = True
    slot[~is_read] = order
    slot[pos] = rng.integers(0, S + 100, nreads)
    value = np.arange(len(kind), dtype=np.int32)
    want = M.arrays(*state_of(gpu), kind, slot, value)              # (the CPU tests hold the two models equal)
    got, _ = call(gpu, kind, slot, value, None, dev=True)
    M.assert_same(got, want)
    assert got.counts[3] - got.counts[2] == span and got.counts[1] > 3000
    assert len(np.unique(got.exec_count[got.exec_count >= 0])) > 100
    gpu.close()


@pytest.mark.parametrize("dev", [False, True])
def test_an_empty_span(fa, dev):
    gpu = context(fa)
    run(gpu, *burst_of([(CH, 0, 1), (CH, 1, 2), (CH, 5, 6)]), dev=dev)
    got = run(gpu, *burst_of([(RD, 0, 0), (CH, 5, 7), (RD, 2, 0), (CH, 4, 5), (RD, 5, 0), (EV, 0, 0), (RD, 1, 0)]), dev=dev)
    assert got.counts == (5, 3, 2, 2) and got.exec_count.tolist() == [2, -2, -1, -2, -1, 2, 2]
    assert got.order.tolist() == [0, 5, 6, 2, 4]
    got = run(gpu, *burst_of([(RD, 2, 0), (EV, 0, 0)]), dev=dev)     # no Chosen at all
    assert got.counts == (2, 1, 2, 2) and got.order.tolist() == [1, 0]
    gpu.close()


def test_a_bad_chosen_slot_is_refused_and_nothing_is_touched(fa):
    import torch

    b = RS.make(3, 256)
    gpu, twin = primed(fa, b), primed(fa, b)
    before = state_of(gpu)
    live = np.flatnonzero((b.kind == CH) & (b.mask != 0))
    slot = b.slot.copy()
    slot[live[40]], slot[live[17]], slot[live[90]] = -1, b.num_slots, 2**31 - 1
    marks = [np.full(256, -9, np.int32) for _ in range(3)]
    st, ec, rs, od, counts, wm, nc = gpu.replica_inbox(b.kind, slot, b.value, b.mask, *marks)
    assert st == EINVAL and gpu.error_detail()[0] == live[17] and (wm, nc) == before[2:] == gpu.replica_state()
    assert all((m == -9).all() for m in marks) and (counts == -9).all()
    got, outs = call(gpu, b.kind, slot, b.value, b.mask, dev=True)
    assert (got.status, got.bad_index) == (EINVAL, live[17]) and all((o == -9).all() for o in outs)
    after = state_of(gpu)
    assert after[2:] == before[2:]
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    # masked out, the bad messages do not count; and the claim words were left clean: the next call equals a twin's
    mask = b.mask.copy()
    mask[live[[40, 17, 90]]] = 0
    got = run(gpu, b.kind, slot, b.value, mask)
    M.assert_same(got, run(twin, b.kind, slot, b.value, mask))
    # refused at once
    lib, h = fa.lib(), gpu._h
    p = torch.zeros(8, dtype=torch.int32, device="cuda").data_ptr()
    for k in range(3):
        args = [None if j == k else p for j in range(3)]
        assert lib.fpx_replica_inbox_dev(h, 4, *args, None, p, p, p, p) == EINVAL
        assert lib.fpx_replica_inbox(h, 4, *[None if a is None else marks[0].ctypes.data for a in args], None,
                                     *[marks[0].ctypes.data] * 4, None, None) == EINVAL
    assert lib.fpx_replica_inbox_dev(h, 4, p, p, p, None, p, None, p, p) == EINVAL      # some outputs but not all
    assert lib.fpx_replica_inbox_dev(h, -1, p, p, p, None, p, p, p, p) == EINVAL
    assert lib.fpx_replica_inbox_dev(h, 1 << 30, p, p, p, None, p, p, p, p) == EINVAL
    assert lib.fpx_replica_inbox_dev(h, 0, None, None, None, None, None, None, None, None) == 0
    assert gpu.sync() == 0 and gpu.replica_state() == (got.w1, got.num_chosen)
    gpu.close(), twin.close()


@pytest.mark.parametrize("outputs", [False, True])
def test_chosen_only_bursts_equal_fpx_replica_chosen_msgs(fa, outputs):
    import torch

    gpu, twin = context(fa), context(fa)
    rng = np.random.default_rng(4)
    for n in (1, 300, 2000):
        slot = rng.integers(0, 1500, n).astype(np.int32)
        slot[: n // 3] = np.arange(n // 3) + (0 if n < 2000 else 250)
        kind = np.where(rng.random(n) < 0.9, CH, wire.PHASE2B).astype(np.int32)
        value, mask = rng.integers(0, 1 << 30, n).astype(np.int32), (rng.random(n) < 0.9).astype(np.uint8)
        want = twin.replica_chosen_msgs(kind, slot, slot, value, mask)
        if outputs:
            got = run(gpu, kind, slot, value, mask, dev=True)
            assert got.counts[:2] == (0, 0) and (got.exec_count == -2).all()
        else:
            gpu.replica_inbox_dev(*[torch.from_numpy(a).cuda() for a in (kind, slot, value, mask)])
            assert gpu.sync() == 0
        assert (0,) + gpu.replica_state() == want
        for a, b in zip(gpu.replica_read_log(0, S0), twin.replica_read_log(0, S0)):
            np.testing.assert_array_equal(a, b)
    gpu.close(), twin.close()


def test_a_mencius_context_is_refused(fa):
    import torch

    gpu = context(fa, num_leader_groups=4)
    k, s, v, _ = burst_of([(CH, 0, 1), (RD, 0, 0)])
    st = gpu.replica_inbox(k, s, v)[0]
    assert st == EINVAL and gpu.replica_state() == (0, 0)
    d = [torch.from_numpy(a).cuda() for a in (k, s, v)]
    assert fa.lib().fpx_replica_inbox_dev(gpu._h, 2, *[t.data_ptr() for t in d], None, None, None, None, None) == EINVAL
    assert gpu.sync() == 0
    gpu.close()


def test_the_scratch_is_counted_and_kept(fa):
    gpu = context(fa)
    before = gpu.device_bytes
    run(gpu, *burst_of(PINNED))
    after = gpu.device_bytes
    assert after - before >= 4 * S0 + 20 * 4            # the claim words and the call's scratch
    run(gpu, *burst_of(BURST))
    assert gpu.device_bytes == after                    # nothing new for a burst that fits
    gpu.close()


def test_the_jni_native_on_the_mock_jvm(fa, jvm):  # noqa: F811
    cfg = np.array([S0, 3, 1, 1, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0], np.int32)   # the 15 fpx_config fields
    h = jvm.call("create", C.c_int64, jvm.arr(cfg))
    assert h > 0
    gpu = context(fa)
    state, counts = jvm.arr(np.zeros(2, np.int32)), jvm.arr(np.zeros(4, np.int32))

    def native(msgs, short=None):
        k, s, v, m = burst_of(msgs)
        n = len(msgs)
        arrs = [k, s, v, m.view(np.int8)] + [np.full(n, -9, np.int32) for _ in range(3)]
        if short is not None:
            arrs[short] = arrs[short][:-1]
        handles = [jvm.arr(a) for a in arrs]
        st = jvm.call("replicaInbox", C.c_int32, h, n, *handles, counts, state)
        return st, [jvm.read(a, np.int32, len(arrs[4 + j])) for j, a in enumerate(handles[4:])]

    for msgs in (PINNED, BURST):
        st, (ec, rs, od) = native(msgs)
        want = call(gpu, *burst_of(msgs))[0]
        got_counts = tuple(int(c) for c in jvm.read(counts, np.int32, 4))
        assert st == 0 and got_counts == want.counts
        assert tuple(jvm.read(state, np.int32, 2)) == (want.w1, want.num_chosen)
        np.testing.assert_array_equal(ec, want.exec_count)
        np.testing.assert_array_equal(rs, want.reply_slot)
        np.testing.assert_array_equal(od[:got_counts[0]], want.order)
    assert ec.tolist() == WANT_EXEC and rs.tolist() == WANT_REPLY
    for short in range(7):                                          # a short array is refused before native code runs
        assert native([(CH, 100, 1), (RD, 100, 0)], short)[0] == EINVAL
    st, outs = native([(CH, 7, 1), (CH, S0, 2)])                    # a bad slot: the arrays are left as they were
    assert st == EINVAL and all((o == -9).all() for o in outs)
    assert jvm.call("destroy", C.c_int32, h) == 0
    gpu.close()
