"""fpx_mencius_acceptor_inbox / _dev (include/fpx.h): a burst of per-acceptor Mencius AcceptorInbound messages, Phase2as,
Phase2aNoopRanges and Phase1as interleaved, in one device call.  For every stream of
tests/mencius_acceptor_inbox_streams.py, both forms:
  (a) the replies equal the message-at-a-time model of tests/mencius_acceptor_inbox_model.py (oracle/mencius_maps.Acceptor);
  (b) state_digest, read_scalars and read_state equal a second context driven one message at a time through the existing
      fpx_acceptor_phase2a / fpx_acceptor_phase2a_noop_range / fpx_acceptor_phase1a with single-bit masks;
  (c) a follow-up burst whose rounds start below where the first ended also agrees;
  (d) a following acceptor_phase1b_info_all, a fused step and fused noop ranges in fresh rounds agree on both contexts (a
      row the burst voted in but did not mark would be written whole by that step, a stale fold would show in a Nack).
tests/test_mencius_acceptor_inbox_cpu.py holds that the streams reach every branch.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import mencius_acceptor_inbox_model as M
from tests import mencius_acceptor_inbox_streams as MS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL = 1
P2A, NR, P1A, OTHER = M.P2A, M.NR, M.P1A, M.OTHER
NAMES = [nm for nm, _, _ in MS.NAMED + MS.SMALL]


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def context(fa, b, **more):
    return fa.Context(fa.make_config(**dict(b.config(), tally_ways=4, **more)))


def model_of(b):
    return M.Sequential(b.L, b.A, b.R, b.S)


def call(gpu, b, dev, replies=True):
    """one burst: (status, reply_kind, reply_value); outputs start as -9"""
    if not dev:
        kind, acc, slot, end, rnd, value, group = b.arrays()
        return gpu.mencius_acceptor_inbox(kind, acc, slot, end, rnd, value, group, replies=replies)
    import torch

    n = len(b)
    kind, acc, slot, end, rnd, value, group = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in b.arrays())
    rk, rv = (torch.full((max(n, 1),), -9, dtype=torch.int32, device="cuda") if replies else None for _ in range(2))
    gpu.mencius_acceptor_inbox_dev(kind, acc, slot, end, rnd, value, group, rk, rv, n=n)
    st = gpu.sync()
    return (st,) + ((rk.cpu().numpy()[:n], rv.cpu().numpy()[:n]) if replies else (None, None))


def one_by_one(twin, b):
    """the parent's route: every message through fpx_acceptor_phase2a / fpx_acceptor_phase2a_noop_range /
    fpx_acceptor_phase1a with a single-bit mask; -> (reply_kind, reply_value)"""
    n = len(b)
    rk, rv = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for i in range(n):
        k = int(b.kind[i])
        if k == OTHER:
            continue
        g, r = int(b.group[i]), int(b.acceptor[i])
        mask = np.zeros((1, 4), np.uint64)
        mask[0, r >> 6] = np.uint64(1) << np.uint64(r & 63)
        if k == P2A:
            st, vb, nb, nr = twin.acceptor_phase2a(b.slot[i:i + 1], b.round[i:i + 1], b.value[i:i + 1], mask)
            assert st == 0 and (vb | nb == mask).all() and not (vb & nb).any()
            rk[i], rv[i] = (M.PHASE2B, b.round[i]) if vb.any() else (M.NACK, nr[0])
        elif k == NR:
            masks = np.zeros((b.A, 4), np.uint64)
            masks[g % b.A] = mask[0]
            st, vb, nb, nr = twin.acceptor_phase2a_noop_range(int(b.slot[i]), int(b.slot_end[i]), int(b.round[i]), masks)
            assert st == 0 and (vb | nb == masks).all() and not (vb & nb).any()
            rk[i], rv[i] = (M.PHASE2B_NR, b.round[i]) if vb.any() else (M.NACK, nr)
        else:
            st, pb, nb = twin.acceptor_phase1a(g, int(b.round[i]), 0, mask[0])
            assert st == 0 and (pb | nb == mask[0]).all()
            rk[i], rv[i] = (M.PHASE1B, b.round[i]) if pb.any() else (M.NACK, twin.read_scalars()[0][g, r])
    return rk, rv


def assert_same_contexts(gpu, twin, what):
    np.testing.assert_array_equal(gpu.state_digest(), twin.state_digest(), err_msg="%s digest" % (what,))
    for a, b, name in zip(gpu.read_scalars() + gpu.read_state()[:2], twin.read_scalars() + twin.read_state()[:2],
                          ("promised", "max_voted", "vote_round", "vote_value")):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, name))


def assert_equals_model(gpu, model, what):
    for a, b, name in zip(gpu.read_scalars() + gpu.read_state()[:2], model.scalars() + model.cells(),
                          ("promised", "max_voted", "vote_round", "vote_value")):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, name))


def burst_on_both(gpu, twin, model, b, dev, what):
    st, bad, want_kind, want_value = model.run(b)
    assert st == 0
    st, rk, rv = call(gpu, b, dev)
    assert st == 0, (what, gpu.error_detail())
    np.testing.assert_array_equal(rk, want_kind, err_msg="%s reply_kind" % (what,))          # (a)
    np.testing.assert_array_equal(rv, want_value, err_msg="%s reply_value" % (what,))
    tk, tv = one_by_one(twin, b)
    np.testing.assert_array_equal(tk, want_kind, err_msg="%s one by one" % (what,))
    np.testing.assert_array_equal(tv, want_value, err_msg="%s one by one" % (what,))
    assert_same_contexts(gpu, twin, what)                                                     # (b)
    assert_equals_model(gpu, model, what)


def afterwards(gpu, twin, b, round_):
    """(d): Phase1b.info of everybody, then a fused step in a round nobody has seen to the lower half of every group, then
    fused noop ranges over every leader group's second half in a round above that"""
    for x, y in zip(gpu.acceptor_phase1b_info_all(0), twin.acceptor_phase1b_info_all(0)):
        np.testing.assert_array_equal(x, y)
    half = (b.R + 1) // 2
    slot = np.arange(b.S, dtype=np.int32)
    mask = np.zeros((b.S, 4), np.uint64)
    for r in range(half):
        mask[:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    outs = [c.phase2_fused(slot, np.full(b.S, round_, np.int32), slot + 5000, mask) for c in (gpu, twin)]
    assert outs[0][0] == outs[1][0] == 0
    for x, y in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(x, y)
    assert (outs[0][4] == -1).all()                                    # nobody Nacks the new round
    assert_same_contexts(gpu, twin, "after the fused step")
    vr = gpu.read_state()[0]
    assert (vr[:, half:] != round_).all() and (vr[:, :half] == round_).all()
    start = (b.S // 2) - (b.S // 2) % b.L + np.arange(b.L, dtype=np.int32)
    outs = [c.noop_ranges_fused(start, np.full(b.L, b.S, np.int32), np.full(b.L, round_ + 1, np.int32)) for c in (gpu, twin)]
    assert outs[0][0] == outs[1][0] == 0
    for x, y in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(x, y)
    assert_same_contexts(gpu, twin, "after the fused ranges")
    vr, vv = gpu.read_state()[:2]
    assert (vr[int(start[0]):] == round_ + 1).all() and (vv[int(start[0]):] == -1).all()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_streams_equal_the_model_and_the_message_at_a_time_route(fa, name, dev):
    b = MS.named(name)
    gpu, twin, model = context(fa, b), context(fa, b), model_of(b)
    burst_on_both(gpu, twin, model, b, dev, name)
    burst_on_both(gpu, twin, model, MS.follow_up(name), dev, name + " follow-up")             # (c)
    afterwards(gpu, twin, b, 900)
    gpu.close(), twin.close()


@pytest.mark.parametrize("dev", [False, True])
def test_a_fused_step_left_pending_before_the_burst(fa, dev):
    """the burst reads promised and max_voted: it must come behind the fold of the fused step enqueued before it"""
    import torch

    b = MS.named("L2_A3_R65")
    gpu, twin, model = context(fa, b), context(fa, b), model_of(b)
    slot = np.arange(b.S, dtype=np.int32)
    for c in (gpu, twin):
        d = [torch.from_numpy(a).cuda() for a in (slot, np.full(b.S, 3, np.int32), slot + 7000)]
        outs = [torch.zeros(b.S, dtype=t, device="cuda") for t in (torch.uint8, torch.int32, torch.int32, torch.int32)]
        c.phase2_fused_dev(*d, None, *outs)                            # no sync: whatever the step deferred is still deferred
    for (lg, ag, r), acc in model.acceptors.items():                   # the step, in the model: everybody votes in round 3
        for s in range(b.S):
            if s % b.L == lg and (s // b.L) % b.A == ag:
                assert acc.handle_phase2a(s, 3, s + 7000) == ("phase2b",)
                model.max_voted[lg, ag, r] = s
    burst_on_both(gpu, twin, model, b, dev, "behind a fused step")
    afterwards(gpu, twin, b, 901)
    gpu.close(), twin.close()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", ["n3000", "L3_A3", "L1_A1"])
def test_a_bad_message_refuses_the_whole_burst(fa, name, dev):
    b = MS.named(name)
    gpu, twin, model = context(fa, b), context(fa, b), model_of(b)
    burst_on_both(gpu, twin, model, b.cut(0, 300), dev, "before")
    before = gpu.state_digest()
    cases = MS.spoiled(b)
    assert len(cases) == 7 + (b.L * b.A > 1) + (b.L > 1)
    for what, c, at in cases:
        st, rk, rv = call(gpu, c, dev)
        assert st == EINVAL and gpu.error_detail()[0] == at, (what, st, gpu.error_detail())
        assert (rk == -9).all() and (rv == -9).all(), what
        np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=what)
    # the scratch was handed back clean: the next burst equals the model and the twin
    burst_on_both(gpu, twin, model, b.cut(300, len(b)), dev, "after")
    gpu.close(), twin.close()


def test_contexts_and_arguments_refused_at_once(fa):
    import torch

    b = MS.named("n257")
    lib = fa.lib()
    p = torch.zeros(512, dtype=torch.int32, device="cuda").data_ptr()
    h = np.zeros(512, np.int32).ctypes.data
    grid = dict(num_replicas=4, f=1, quorum_kind=2, grid_rows=2, grid_cols=2)
    for more in (dict(ballot_mode=fa.FPX_BALLOT_PER_SLOT), grid):                           # a ballot per cell; a grid quorum
        gpu = context(fa, b, **more)
        before = gpu.state_digest()
        assert call(gpu, b, False)[0] == EINVAL
        assert lib.fpx_mencius_acceptor_inbox_dev(gpu._h, 4, p, p, p, p, p, p, p, p, p) == EINVAL
        assert gpu.sync() == 0
        np.testing.assert_array_equal(gpu.state_digest(), before)
        gpu.close()
    gpu = context(fa, b)
    for k in (0, 2, 3, 4, 5, 6):                                                            # group_index alone may be NULL
        args = [None if j == k else p for j in range(7)]
        assert lib.fpx_mencius_acceptor_inbox_dev(gpu._h, 4, *args, p, p) == EINVAL
        assert lib.fpx_mencius_acceptor_inbox(gpu._h, 4, *[None if a is None else h for a in args], h, h) == EINVAL
    for n in (-1, 1 << 30):
        assert lib.fpx_mencius_acceptor_inbox_dev(gpu._h, n, p, p, p, p, p, p, p, p, p) == EINVAL
        assert lib.fpx_mencius_acceptor_inbox(gpu._h, n, h, h, h, h, h, h, h, h, h) == EINVAL
    assert lib.fpx_mencius_acceptor_inbox_dev(gpu._h, 0, *[None] * 7, None, None) == 0
    assert lib.fpx_mencius_acceptor_inbox(gpu._h, 0, *[None] * 7, None, None) == 0
    assert gpu.sync() == 0
    gpu.close()
    # num_leader_groups == 1 and one acceptor group are allowed; the MultiPaxos call still refuses a Mencius context
    gpu = context(fa, MS.named("n256"))
    assert lib.fpx_acceptor_inbox(gpu._h, 4, h, h, h, h, h, h, 0, h, h) == EINVAL
    gpu.close()


@pytest.mark.parametrize("dev", [False, True])
def test_null_outputs(fa, dev):
    b = MS.named("L3_A2_R4")
    gpu, twin, model = context(fa, b), context(fa, b), model_of(b)
    assert call(gpu, b, dev, replies=False) == (0, None, None)
    one_by_one(twin, b)
    model.run(b)
    assert_same_contexts(gpu, twin, "no outputs")
    assert_equals_model(gpu, model, "no outputs")
    # one output only; group_index NULL on a context of one group
    f = MS.follow_up("L3_A2_R4")
    kind, acc, slot, end, rnd, value, group = f.arrays()
    want = model.run(f)
    rk = np.full(len(f), -9, np.int32)
    assert fa.lib().fpx_mencius_acceptor_inbox(gpu._h, len(f), *(a.ctypes.data for a in (kind, group, acc, slot, end, rnd, value)),
                                               rk.ctypes.data, None) == 0
    np.testing.assert_array_equal(rk, want[2])
    gpu.close(), twin.close()
    b = MS.named("n255")
    gpu, model = context(fa, b), model_of(b)
    want = model.run(b)
    kind, acc, slot, end, rnd, value, group = b.arrays()
    assert (group[b.kind != OTHER] == 0).all()
    st, rk, rv = gpu.mencius_acceptor_inbox(kind, acc, slot, end, rnd, value, None)
    assert st == 0
    np.testing.assert_array_equal(rk, want[2]), np.testing.assert_array_equal(rv, want[3])
    gpu.close()


def test_a_torch_stream_other_than_the_default(fa):
    import torch

    b = MS.named("L1_A3_R4")
    gpu, model = context(fa, b), model_of(b)
    side = torch.cuda.Stream()
    gpu.set_stream(side.cuda_stream)
    with torch.cuda.stream(side):
        for burst in (b, MS.follow_up("L1_A3_R4")):
            st, bad, want_kind, want_value = model.run(burst)
            st, rk, rv = call(gpu, burst, True)
            assert st == 0
            np.testing.assert_array_equal(rk, want_kind)
            np.testing.assert_array_equal(rv, want_value)
    assert_equals_model(gpu, model, "side stream")
    gpu.close()


def test_the_scratch_is_counted_and_kept(fa):
    b = MS.named("n3000")
    gpu = context(fa, b)
    before = gpu.device_bytes
    assert call(gpu, b, False)[0] == 0
    after = gpu.device_bytes
    assert after - before >= 12 * 8192 + 48 * 3000                     # the claim table of 2^13 words and the call's scratch
    assert call(gpu, MS.follow_up("n3000"), True)[0] == 0
    assert gpu.device_bytes == after                                   # nothing new for a burst that fits
    gpu.close()


def test_the_jni_native_on_the_mock_jvm(fa, jvm):  # noqa: F811
    b = MS.named("n3000")
    cfg = np.array([b.S, b.R, b.A, b.L, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0], np.int32)      # the 15 fpx_config fields
    h = jvm.call("create", C.c_int64, jvm.arr(cfg))
    assert h > 0
    gpu = context(fa, b)

    def native(burst, short=None, outputs=True):
        n = len(burst)
        kind, acc, slot, end, rnd, value, group = burst.arrays()
        arrs = [kind, group, acc, slot, end, rnd, value, np.full(n, -9, np.int32), np.full(n, -9, np.int32)]
        if short is not None:
            arrs[short] = arrs[short][:-1]
        handles = [jvm.arr(a) for a in arrs]
        if not outputs:
            handles[7] = handles[8] = None
        st = jvm.call("menciusAcceptorInbox", C.c_int32, h, n, *handles)
        return st, [jvm.read(a, np.int32, len(arrs[7 + j])) for j, a in enumerate(handles[7:]) if a is not None]

    for burst in (b, MS.follow_up("n3000")):
        st, (rk, rv) = native(burst)
        want = call(gpu, burst, False)
        assert st == want[0] == 0
        np.testing.assert_array_equal(rk, want[1])
        np.testing.assert_array_equal(rv, want[2])
    for short in range(9):                                             # a short array is refused before native code runs
        assert native(b.cut(0, 50), short)[0] == EINVAL
    what, c, at = MS.spoiled(b)[4]                                     # a bad slot: the arrays are left as they were
    st, outs = native(c)
    assert st == EINVAL and all((o == -9).all() for o in outs)
    assert native(b.cut(0, 50), outputs=False)[0] == 0 and call(gpu, b.cut(0, 50), False, replies=False)[0] == 0
    assert jvm.call("destroy", C.c_int32, h) == 0
    gpu.close()


def test_a_gpu_mencius_acceptor_shaped_walk_on_wire_bytes(fa):
    """AcceptorInbound bytes -> fpx_wire_mencius_decode_acceptor_inbound -> the inbox -> ProxyLeaderInbound{Phase2b /
    Phase2bNoopRange} / LeaderInbound{Nack} bytes by the existing encoders, as jni/MenciusNative.scala's GpuMenciusAcceptor
    walks a burst.  L = 2, A = 2, R = 3: leader group 1's acceptor groups own slots 1, 5, 9, ... and 3, 7, 11, ..."""
    L, A, R, S = 2, 2, 3, 64
    cmd = bytes.fromhex("0a00")
    enc = wire.mencius_encode
    # (bytes, leader group, acceptor group, acceptor it was delivered to)
    msgs = [(enc("acceptor_phase2a", 5, 2, cmd), 1, 0, 1), (enc("acceptor_phase2a", 5, 2, cmd), 1, 0, 2),
            (enc("acceptor_phase2a_noop_range", 1, 21, 2), 1, 0, 1), (enc("acceptor_phase2a_noop_range", 1, 21, 2), 1, 1, 0),
            (enc("acceptor_phase1a", 4, 0), 1, 0, 1), (enc("acceptor_phase2a", 9, 2, None), 1, 0, 1),
            (enc("acceptor_phase2a_noop_range", 21, 31, 3), 1, 0, 1), (enc("acceptor_phase2a", 13, 4, cmd), 1, 0, 1),
            (enc("acceptor_phase2a_noop_range", 0, 10, 1), 0, 1, 2)]
    d = wire.mencius_decode_acceptor_inbound([m for m, _, _, _ in msgs])
    assert d["status"] == 0 and d["kind"].tolist() == [P2A, P2A, NR, NR, P1A, P2A, NR, P2A, NR]
    n = len(msgs)
    group = np.array([lg * A + ag for _, lg, ag, _ in msgs], np.int32)
    acc = np.array([a for _, _, _, a in msgs], np.int32)
    value = np.where(d["kind"] == P2A, np.where(d["is_noop"] == 1, -1, np.arange(n)), -1).astype(np.int32)
    b = MS.Burst(L, A, R, S, 0, d["kind"], group, acc, d["slot"], d["slot_end"], d["round"], value)
    gpu = context(fa, b)
    st, rk, rv = call(gpu, b, False)
    assert st == 0
    assert rk.tolist() == [M.PHASE2B, M.PHASE2B, M.PHASE2B_NR, M.PHASE2B_NR, M.PHASE1B, M.NACK, M.NACK, M.PHASE2B, M.PHASE2B_NR]
    assert rv.tolist() == [2, 2, 2, 2, 4, 4, 4, 4, 1]
    vr, vv = gpu.read_state()[:2]
    assert [(int(vr[s, 1]), int(vv[s, 1])) for s in (1, 5, 9, 13, 17, 21)] == [(2, -1), (2, -1), (2, -1), (4, 7), (2, -1), (-1, -1)]
    assert (int(vr[5, 2]), int(vv[5, 2])) == (2, 1) and [int(vr[s, 0]) for s in (3, 7, 11, 15, 19, 23)] == [2, 2, 2, 2, 2, -1]
    assert [int(vr[s, 2]) for s in (0, 2, 4, 6, 8, 10)] == [-1, 1, -1, 1, -1, -1]
    out = []
    for i in range(n):
        ag = int(group[i]) % A
        if rk[i] == M.PHASE2B:
            out.append(enc("proxy_leader_phase2b", int(acc[i]), int(d["slot"][i]), int(rv[i])))
        elif rk[i] == M.PHASE2B_NR:
            out.append(enc("proxy_leader_phase2b_noop_range", ag, int(acc[i]), int(d["slot"][i]), int(d["slot_end"][i]), int(rv[i])))
        elif rk[i] == M.NACK:
            # to leader roundSystem.leader(round) of leader group slot % L (mencius/Acceptor.scala:215-218, :250-253)
            out.append((int(d["slot"][i]) % L, fa.round_leader(2, int(d["round"][i])), enc("leader_nack", int(rv[i]))))
    assert len(out) == 8 and out[4][:2] == (1, 0) and out[5][:2] == (1, 1)
    back = wire.mencius_decode_proxy_leader_inbound([o for o in out if isinstance(o, bytes)])
    assert back["status"] == 0
    assert back["kind"].tolist() == [wire.PHASE2B, wire.PHASE2B, wire.PHASE2B_NOOP_RANGE, wire.PHASE2B_NOOP_RANGE, wire.PHASE2B,
                                     wire.PHASE2B_NOOP_RANGE]
    assert back["round"].tolist() == [2, 2, 2, 2, 4, 1] and back["slot"].tolist() == [5, 5, 1, 1, 13, 0]
    gpu.close()
