"""fpx_proxy_phase2b_msgs / _dev and fpx_wire_phase2b_tick (include/fpx.h, include/fpx_wire.h): a tick of per-acceptor
Phase2b messages tallied on the device without a host fold -- against fpx_wire_phase2b_rows + fpx_proxy_phase2b on a
second context (bit for bit) and against the oracle's ProxyLeader.handlePhase2b message at a time (the same values
chosen, each once, the same Pending / Done entries).  The streams are tests/phase2b_streams.py.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from tests import phase2b_streams as PS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL, EUNKNOWN, ECAPACITY = 1, 2, 5
PHASE2A, PHASE2B = 1, 2


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


def context(fa, kw):
    import torch

    gpu = fa.Context(fa.make_config(**kw))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)  # the uploads below are torch's
    return gpu


def rows_path(wire, ref, d, grid_cols):
    """fpx_wire_phase2b_rows + fpx_proxy_phase2b on `ref`, each row's outcome moved to the index of its first message:
    (status, newly_chosen, chosen_round, chosen_value)"""
    n = len(d["kind"])
    ch, cr, cv = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rs, rr, rb = wire.phase2b_rows(d, grid_cols)
    first = {}
    for i in np.nonzero(d["kind"] == PHASE2B)[0].tolist():
        first.setdefault((int(d["slot"][i]), int(d["round"][i])), i)
    at = np.array([first[(int(s), int(r))] for s, r in zip(rs, rr)], np.int64)
    assert (np.diff(at) > 0).all()          # rows come in order of first appearance
    st, rch, rcr, rcv = ref.proxy_phase2b(rs, rr, rb) if len(rs) else (0, [], [], [])
    if len(rs):
        ch[at], cr[at], cv[at] = rch, rcr, rcv
    return st, ch, cr, cv


def dev_call(gpu, d, grid_cols, with_kind=True, with_group=True):
    """fpx_proxy_phase2b_msgs_dev + fpx_sync: (status, newly_chosen, chosen_round, chosen_value)"""
    import torch

    dev = torch.device("cuda:0")
    n = len(d["slot"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    ch = torch.full((max(n, 1),), 77, dtype=torch.uint8, device=dev)[:n]
    cr = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev)[:n]
    cv = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev)[:n]
    gpu.proxy_phase2b_msgs_dev(t["acceptor_index"], t["slot"], t["round"], kind=t["kind"] if with_kind else None,
                               group_index=t["group_index"] if with_group else None, grid_cols=grid_cols,
                               newly_chosen=ch, chosen_round=cr, chosen_value=cv)
    st = gpu.sync()
    return st, ch.cpu().numpy(), cr.cpu().numpy(), cv.cpu().numpy()


def records(d, ch, cr, cv):
    idx = np.nonzero(ch)[0]
    return [(int(i), int(d["slot"][i]), int(cr[i]), int(cv[i])) for i in idx]


def open_all(gpu, st):
    rc, new = gpu.proxy_open(st.open_slot, st.open_round, st.open_value)
    assert rc == 0 and new.all()


def chunks(n):
    """some streams go in two calls: entries stay Pending in between, complete in the second, get votes after Done"""
    return [(0, n)] if n < 64 else [(0, n // 2), (n // 2, n)]


@pytest.mark.parametrize("layout", PS.LAYOUTS)
@pytest.mark.parametrize("shape", sorted(PS.SHAPES))
def test_the_device_tally_equals_the_rows_path_and_the_reference(fa, wire, oracle, shape, layout):
    kw = PS.SHAPES[shape]
    gpu, ref = context(fa, kw), context(fa, kw)
    for n in PS.LENGTHS:
        st = PS.Stream(shape, n, layout, seed=100 + n)
        assert st.n == n
        gpu.reset(), ref.reset()
        open_all(gpu, st), open_all(ref, st)
        got = []
        for lo, hi in chunks(n):
            d = st.decoded(lo, hi)
            # (group_index NULL means 0: only where the shape has no grid)
            rc, ch, cr, cv = dev_call(gpu, d, st.grid_cols, with_kind=(lo == 0), with_group=bool(st.grid_cols) or lo == 0)
            wrc, wch, wcr, wcv = rows_path(wire, ref, d, st.grid_cols)
            assert rc == 0 and wrc == 0
            # 1. the rows path, bit for bit
            assert records(d, ch, cr, cv) == records(d, wch, wcr, wcv)
            np.testing.assert_array_equal(ch, wch), np.testing.assert_array_equal(cr, wcr), np.testing.assert_array_equal(cv, wcv)
            np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
            got += [(s, r, v) for _, s, r, v in records(d, ch, cr, cv)]
        touched = sorted(set(st.slot.tolist()))
        for s in touched:
            assert gpu.read_tally(s) == ref.read_tally(s), "tally of slot %d" % s
        # 2. the reference, message at a time: the same values chosen, each exactly once; the same Pending / Done
        _, chosen, states = PS.oracle_run(oracle, st)
        assert sorted(got) == sorted((s, r, v) for _, s, r, v in chosen) and len(set(got)) == len(got)
        for s in sorted(set(st.open_slot.tolist())):
            for rnd, state, value, bits in gpu.read_tally(s):
                assert states[(s, rnd)] - 1 == state, (s, rnd)   # read_tally: 0 Pending, 1 Done
    gpu.close(), ref.close()


def test_unknown_slotrounds_are_dropped_and_the_lowest_index_is_named(fa, wire):
    st = PS.Stream("r3", 20000, "random", seed=31)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    d = st.decoded()
    lo, hi = 300, 15000                                  # different workgroups, far apart
    d["round"][[lo, hi]] = 9                             # never opened
    rc, ch, cr, cv = dev_call(gpu, d, 0)
    assert rc == EUNKNOWN
    assert gpu.error_detail() == (lo, int(d["slot"][lo]), 9)
    # every other message was applied: the rows path without the two
    d2 = {k: v.copy() for k, v in d.items()}
    d2["kind"][[lo, hi]] = 0
    wrc, wch, wcr, wcv = rows_path(wire, ref, d2, 0)
    assert wrc == 0 and wch.sum() > 0
    np.testing.assert_array_equal(ch, wch), np.testing.assert_array_equal(cr, wcr), np.testing.assert_array_equal(cv, wcv)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


@pytest.mark.parametrize("what", ["bit256", "negative", "beyond_grid_cols", "slot_outside"])
def test_a_bad_message_is_einval_nothing_is_applied_and_the_owner_table_stays_clean(fa, wire, what):
    shape = "grid2x3" if what == "beyond_grid_cols" else "r3"
    st = PS.Stream(shape, 20000, "random", seed=32)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    before = gpu.state_digest()
    d = st.decoded()
    bad = {k: v.copy() for k, v in d.items()}
    at = [9000, 4100]                                    # the lower index is the one named
    if what == "bit256":
        bad["acceptor_index"][at] = 256
    elif what == "negative":
        bad["acceptor_index"][at] = -1
    elif what == "beyond_grid_cols":
        bad["acceptor_index"][at] = 3
    else:
        bad["slot"][at] = st.kw["num_slots"]
    rc, ch, cr, cv = dev_call(gpu, bad, st.grid_cols)
    assert rc == EINVAL and gpu.error_detail()[0] == 4100
    assert not ch.any() and (cr == -1).all() and (cv == -1).all()
    np.testing.assert_array_equal(gpu.state_digest(), before)
    # a correct call straight after gives the right result: no owner word was left behind by the refused call
    rc, ch, cr, cv = dev_call(gpu, d, st.grid_cols)
    wrc, wch, wcr, wcv = rows_path(wire, ref, d, st.grid_cols)
    assert rc == 0 and wrc == 0 and wch.sum() > 0
    np.testing.assert_array_equal(ch, wch), np.testing.assert_array_equal(cr, wcr), np.testing.assert_array_equal(cv, wcv)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


def test_other_kinds_are_skipped_and_an_empty_batch_is_ok(fa, wire):
    st = PS.Stream("ways4", 257, "random", seed=33)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    d = st.decoded()
    rng = np.random.default_rng(5)
    other = rng.random(st.n) < 0.3
    d["kind"][other] = rng.choice([0, PHASE2A, 3, 5], size=int(other.sum()))
    d["slot"][other & (rng.random(st.n) < 0.5)] = -1      # what the decoder leaves in fields that do not apply
    rc, ch, cr, cv = dev_call(gpu, d, 0)
    wrc, wch, wcr, wcv = rows_path(wire, ref, d, 0)
    assert rc == 0 and wrc == 0 and not ch[other].any() and wch.sum() > 0
    np.testing.assert_array_equal(ch, wch), np.testing.assert_array_equal(cr, wcr), np.testing.assert_array_equal(cv, wcv)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    # n == 0
    before = gpu.state_digest()
    assert dev_call(gpu, st.decoded(0, 0), 0)[0] == 0
    assert gpu.proxy_phase2b_msgs(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), before)
    gpu.close(), ref.close()


@pytest.mark.parametrize("shape,n", [("r3", 257), ("grid2x3", 20000), ("r256", 20000), ("lg4", 65)])
def test_the_host_form_equals_the_device_form(fa, shape, n):
    st = PS.Stream(shape, n, "random", seed=34)
    a, b = context(fa, st.kw), context(fa, st.kw)
    open_all(a, st), open_all(b, st)
    total = 0
    for lo, hi in chunks(n):
        d = st.decoded(lo, hi)
        rc, ch, cr, cv = dev_call(a, d, st.grid_cols)
        hrc, hch, hcr, hcv = b.proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"],
                                                  group_index=d["group_index"], grid_cols=st.grid_cols)
        assert rc == 0 and hrc == 0
        total += int(ch.sum())
        np.testing.assert_array_equal(ch, hch), np.testing.assert_array_equal(cr, hcr), np.testing.assert_array_equal(cv, hcv)
        np.testing.assert_array_equal(a.state_digest(), b.state_digest())
    assert total > 0      # (with 128 of 256 votes needed, in random order, the first call alone completes nothing)
    # the host form's errors: the status comes back from the call itself
    d = st.decoded()
    d["acceptor_index"][n // 2] = -1
    before = b.state_digest()
    assert b.proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], group_index=d["group_index"],
                                grid_cols=st.grid_cols)[0] == EINVAL
    assert b.error_detail()[0] == n // 2
    np.testing.assert_array_equal(b.state_digest(), before)
    a.close(), b.close()


# ---- the tick: bytes to records -------------------------------------------------------------------------------------
def tick_bytes(wire, st, rng, lo=0, hi=None):
    """the stream's messages [lo, hi) as ProxyLeaderInbound{Phase2b} bytes with Phase2a messages mixed in"""
    hi = st.n if hi is None else hi
    msgs = []
    for i in range(lo, hi):
        if rng.random() < 0.15:
            msgs.append(wire.encode_proxy_leader_phase2a(int(rng.integers(0, st.kw["num_slots"])), 2, None))
        msgs.append(wire.encode_proxy_leader_phase2b(int(st.group_index[i]), int(st.acceptor_index[i]), int(st.slot[i]),
                                                     int(st.round[i])))
    return msgs


class Pinned:
    """the tick's buffers in fpx_host_alloc memory"""

    def __init__(self, fa, wire, msgs, out_cap):
        from frankenpaxos_amd.context import PinnedArray

        buf, off = wire.pack(msgs)
        self.n, self.in_len, self.out_cap = len(msgs), int(off[-1]), out_cap
        self.keep = [PinnedArray(max(1, self.in_len), np.uint8), PinnedArray(self.n + 1, np.int64)] + \
            [PinnedArray(out_cap + 4, np.int32) for _ in range(3)]
        self.inb, self.ino, self.oslot, self.oround, self.ovalue = (k.array for k in self.keep)
        self.inb[:self.in_len] = buf[:self.in_len]
        self.ino[:] = off
        for o in (self.oslot, self.oround, self.ovalue):
            o[:] = -77

    def run(self, gpu, grid_cols):
        return gpu.wire_phase2b_tick(self.inb.ctypes.data, self.in_len, self.ino.ctypes.data, self.n, self.oslot.ctypes.data,
                                     self.oround.ctypes.data, self.ovalue.ctypes.data, self.out_cap, grid_cols)

    def records(self, count):
        return list(zip(self.oslot[:count].tolist(), self.oround[:count].tolist(), self.ovalue[:count].tolist()))


def expected_records(wire, ref, msgs, grid_cols):
    d = wire.decode_proxy_leader_inbound(msgs)
    assert d["status"] == 0
    wrc, wch, wcr, wcv = rows_path(wire, ref, d, grid_cols)
    assert wrc == 0
    return d, [(s, r, v) for _, s, r, v in records(d, wch, wcr, wcv)]


@pytest.mark.parametrize("shape", ["r3", "grid2x3"])
def test_the_tick_gives_the_records_of_the_rows_path(fa, wire, shape):
    st = PS.Stream(shape, 3000, "random", seed=41)
    rng = np.random.default_rng(42)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    for lo, hi in chunks(st.n):
        msgs = tick_bytes(wire, st, rng, lo, hi)
        d, want = expected_records(wire, ref, msgs, st.grid_cols)
        assert (d["kind"] == PHASE2A).any() and len(want) > 0
        p = Pinned(fa, wire, msgs, out_cap=len(msgs))
        rc, count, bad = p.run(gpu, st.grid_cols)
        assert rc == 0 and bad == -1 and count == len(want)
        assert p.records(count) == want and (p.oslot[p.out_cap:] == -77).all()   # ([count, out_cap) is unspecified)
        np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    # n == 0
    assert Pinned(fa, wire, [], out_cap=4).run(gpu, st.grid_cols) == (0, 0, -1)
    gpu.close(), ref.close()


def test_a_refused_tick_applies_nothing_and_a_small_out_is_ecapacity_with_the_tick_applied(fa, wire):
    st = PS.Stream("r3", 3000, "random", seed=43)
    rng = np.random.default_rng(44)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    before = gpu.state_digest()
    msgs = tick_bytes(wire, st, rng)
    # a truncated message
    cut = list(msgs)
    cut[1234] = cut[1234][:-1]
    rc, count, bad = Pinned(fa, wire, cut, out_cap=len(cut)).run(gpu, 0)
    assert rc == EINVAL and bad == 1234 and count == 0
    np.testing.assert_array_equal(gpu.state_digest(), before)
    # pageable memory
    buf, off = wire.pack(msgs)
    out = np.zeros(len(msgs), np.int32)
    assert gpu.wire_phase2b_tick(buf.ctypes.data, int(off[-1]), off.ctypes.data, len(msgs), out.ctypes.data, out.ctypes.data,
                                 out.ctypes.data, len(out))[0] == EINVAL
    np.testing.assert_array_equal(gpu.state_digest(), before)
    # too small an out: the tick is applied, the count needed comes back
    d, want = expected_records(wire, ref, msgs, 0)
    p = Pinned(fa, wire, msgs, out_cap=len(want) - 1)
    rc, count, bad = p.run(gpu, 0)
    assert rc == ECAPACITY and count == len(want)
    assert p.records(len(want) - 1) == want[:-1] and (p.oslot[len(want) - 1:] == -77).all()
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


def test_the_jni_native_tallies_the_same_tick(fa, wire, jvm):  # noqa: F811
    st = PS.Stream("grid2x3", 3000, "random", seed=45)
    rng = np.random.default_rng(46)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    open_all(gpu, st), open_all(ref, st)
    msgs = tick_bytes(wire, st, rng)
    d, want = expected_records(wire, ref, msgs, st.grid_cols)
    n = len(msgs)
    h = gpu._h.value if hasattr(gpu._h, "value") else int(gpu._h)
    arrs = [jvm.arr(d[k]) for k in ("kind", "group_index", "acceptor_index", "slot", "round")]
    ch, cr, cv = jvm.arr(np.zeros(n, np.int8)), jvm.arr(np.zeros(n, np.int32)), jvm.arr(np.zeros(n, np.int32))
    call = lambda *a: jvm.call("proxyPhase2bMsgs", C.c_int32, C.c_int64(h), *a)
    # the array-length checks every native has
    short = jvm.arr(np.zeros(n - 1, np.int32))
    assert call(n, arrs[0], arrs[1], short, arrs[3], arrs[4], st.grid_cols, ch, cr, cv) == EINVAL
    assert call(n, arrs[0], arrs[1], arrs[2], arrs[3], arrs[4], st.grid_cols, ch, short, cv) == EINVAL
    assert call(n, arrs[0], arrs[1], None, arrs[3], arrs[4], st.grid_cols, ch, cr, cv) == EINVAL
    assert call(n, *arrs, st.grid_cols, ch, cr, cv) == 0
    gch, gcr, gcv = jvm.read(ch, np.int8, n), jvm.read(cr, np.int32, n), jvm.read(cv, np.int32, n)
    assert [(s, r, v) for _, s, r, v in records(d, gch, gcr, gcv)] == want and len(want) > 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()
