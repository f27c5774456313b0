"""fpx_acceptor_inbox / _dev (include/fpx.h): a burst of per-acceptor AcceptorInbound messages, the kinds interleaved, in one
device call.  For every stream of tests/acceptor_inbox_streams.py, both forms:
  (a) the replies equal the message-at-a-time model of tests/acceptor_inbox_model.py (oracle/multipaxos_maps.Acceptor);
  (b) state_digest, read_scalars and read_state equal a second context driven one message at a time through the existing
      fpx_acceptor_phase2a / fpx_acceptor_phase1a with single-bit masks;
  (c) a following acceptor_phase1b_info_all and a following fused step to half of every group agree on both contexts
      (a row the burst voted in but did not mark would be written whole by that step, a stale fold would show in a Nack).
tests/test_acceptor_inbox_cpu.py holds that the streams reach every branch.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import acceptor_inbox_model as M
from tests import acceptor_inbox_streams as AS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL = 1
P2A, P1A, MSR, BMSR, OTHER = M.P2A, M.P1A, M.MSR, M.BMSR, M.OTHER
NAMES = [nm for nm, _, _ in AS.NAMED + AS.SMALL]


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def context(fa, b, **more):
    return fa.Context(fa.make_config(**dict(b.config(), tally_ways=4, **more)))


def call(gpu, b, dev, replies=True, stream=None):
    """one burst: (status, reply_kind, reply_value); outputs start as -9"""
    if not dev:
        kind, acc, slot, rnd, value, group = b.arrays()
        return gpu.acceptor_inbox(kind, acc, slot, rnd, value, group, b.grid_cols, replies=replies)
    import torch

    n = len(b)
    kind, acc, slot, rnd, value, group = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in b.arrays())
    rk, rv = (torch.full((max(n, 1),), -9, dtype=torch.int32, device="cuda") if replies else None for _ in range(2))
    gpu.acceptor_inbox_dev(kind, acc, slot, rnd, value, group, b.grid_cols, rk, rv, n=n)
    st = gpu.sync()
    return (st,) + ((rk.cpu().numpy()[:n], rv.cpu().numpy()[:n]) if replies else (None, None))


def one_by_one(twin, b):
    """the parent's route: every message through fpx_acceptor_phase2a / fpx_acceptor_phase1a with a single-bit mask (the
    reads from fpx_read_scalars); -> (reply_kind, reply_value)"""
    n = len(b)
    rk, rv = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for i in range(n):
        k = int(b.kind[i])
        if k == OTHER:
            continue
        g, r = M.entry_of(b, i)
        mask = np.zeros((1, 4), np.uint64)
        mask[0, r >> 6] = np.uint64(1) << np.uint64(r & 63)
        if k == P2A:
            st, vb, nb, nr = twin.acceptor_phase2a(b.slot[i:i + 1], b.round[i:i + 1], b.value[i:i + 1], mask)
            assert st == 0 and (vb | nb == mask).all() and not (vb & nb).any()
            rk[i], rv[i] = (M.PHASE2B, b.round[i]) if vb.any() else (M.NACK, nr[0])
        elif k == P1A:
            st, pb, nb = twin.acceptor_phase1a(g, int(b.round[i]), 0, mask[0])
            assert st == 0 and (pb | nb == mask[0]).all()
            rk[i], rv[i] = (M.PHASE1B, b.round[i]) if pb.any() else (M.NACK, twin.read_scalars()[0][g, r])
        else:
            rk[i], rv[i] = MSR, twin.read_scalars()[1][g, r]
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
    """(c): Phase1b.info of everybody, then a fused step in a round nobody has seen to the lower half of every group"""
    for x, y in zip(gpu.acceptor_phase1b_info_all(0), twin.acceptor_phase1b_info_all(0)):
        np.testing.assert_array_equal(x, y)
    slot = np.arange(b.S, dtype=np.int32)
    mask = np.zeros((b.S, 4), np.uint64)
    for r in range((b.R + 1) // 2):
        mask[:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    outs = [c.phase2_fused(slot, np.full(b.S, round_, np.int32), slot + 5000, mask) for c in (gpu, twin)]
    assert outs[0][0] == outs[1][0] == 0
    for x, y in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(x, y)
    assert (outs[0][4] == -1).all()                                    # nobody Nacks the new round
    assert_same_contexts(gpu, twin, "after the fused step")
    vr = gpu.read_state()[0]
    assert (vr[:, (b.R + 1) // 2:] != round_).all() and (vr[:, :(b.R + 1) // 2] == round_).all()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_streams_equal_the_model_and_the_message_at_a_time_route(fa, name, dev):
    b = AS.named(name)
    gpu, twin, model = context(fa, b), context(fa, b), M.Sequential(b.R, b.groups, b.S)
    burst_on_both(gpu, twin, model, b, dev, name)
    burst_on_both(gpu, twin, model, AS.follow_up(name), dev, name + " follow-up")
    afterwards(gpu, twin, b, 900)
    gpu.close(), twin.close()


def test_a_burst_that_takes_the_one_workgroup_scans_past_their_first_step(fa):
    """n = 1024 * 256 + 3 * 256 + 57 messages are 1028 tiles: the sort's count scan (fpx_burst_sort.hpp, 8192 counts a
    step) has 16 * 1028 = 16 448 counts, three steps, and the 64-bit tile scan (1024 tiles a step) two -- the carry of
    scan_array_excl (fpx_scan.hpp) in both instantiations.  Against the model only: the message-at-a-time twin would
    take minutes here"""
    n = 1024 * 256 + 3 * 256 + 57
    b = AS.make(21, n=n, R=3, S=4096)
    gpu, model = context(fa, b), M.Sequential(b.R, b.groups, b.S)
    st, bad, want_kind, want_value = model.run(b)
    assert st == 0
    for k in (M.PHASE2B, M.PHASE1B, M.NACK, MSR):                      # every reply kind, and both kinds of read
        assert (want_kind == k).sum() >= 1000, k
    assert (b.kind == MSR).sum() >= 1000 and (b.kind == BMSR).sum() >= 1000
    st, rk, rv = call(gpu, b, True)
    assert st == 0, gpu.error_detail()
    np.testing.assert_array_equal(rk, want_kind)
    np.testing.assert_array_equal(rv, want_value)
    assert_equals_model(gpu, model, "n = %d" % n)
    gpu.close()


@pytest.mark.parametrize("dev", [False, True])
def test_a_fused_step_left_pending_before_the_burst(fa, dev):
    """the burst reads promised and max_voted: it must come behind the fold of the fused step enqueued before it"""
    import torch

    b = AS.named("R65")
    gpu, twin, model = context(fa, b), context(fa, b), M.Sequential(b.R, b.groups, b.S)
    slot = np.arange(b.S, dtype=np.int32)
    for c in (gpu, twin):
        d = [torch.from_numpy(a).cuda() for a in (slot, np.full(b.S, 3, np.int32), slot + 7000)]
        outs = [torch.zeros(b.S, dtype=t, device="cuda") for t in (torch.uint8, torch.int32, torch.int32, torch.int32)]
        c.phase2_fused_dev(*d, None, *outs)                            # no sync: whatever the step deferred is still deferred
    for acc in model.acceptors.values():                               # the step, in the model: everybody votes in round 3
        for s in range(b.S):
            assert acc.handle_phase2a(s, 3, s + 7000) == ("phase2b",)
    burst_on_both(gpu, twin, model, b, dev, "behind a fused step")
    afterwards(gpu, twin, b, 901)
    gpu.close(), twin.close()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", ["n3000", "groups3", "grid2x2"])
def test_a_bad_message_refuses_the_whole_burst(fa, name, dev):
    b = AS.named(name)
    gpu, twin, model = context(fa, b), context(fa, b), M.Sequential(b.R, b.groups, b.S)
    burst_on_both(gpu, twin, model, b.cut(0, 300), dev, "before")
    before = gpu.state_digest()
    for what, c, at in AS.spoiled(b):
        st, rk, rv = call(gpu, c, dev)
        assert st == EINVAL and gpu.error_detail()[0] == at, (what, st, gpu.error_detail())
        assert (rk == -9).all() and (rv == -9).all(), what
        np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=what)
    # the scratch was handed back clean: the next burst equals the model and the twin
    burst_on_both(gpu, twin, model, b.cut(300, len(b)), dev, "after")
    gpu.close(), twin.close()


def test_contexts_and_arguments_refused_at_once(fa):
    import torch

    b = AS.named("n257")
    lib = fa.lib()
    p = torch.zeros(512, dtype=torch.int32, device="cuda").data_ptr()
    h = np.zeros(512, np.int32).ctypes.data
    for more in (dict(ballot_mode=fa.FPX_BALLOT_PER_SLOT), dict(num_leader_groups=4)):      # a ballot per cell; Mencius
        gpu = context(fa, b, **more)
        before = gpu.state_digest()
        assert call(gpu, b, False)[0] == EINVAL
        assert lib.fpx_acceptor_inbox_dev(gpu._h, 4, p, p, p, p, p, p, 0, p, p) == EINVAL
        assert gpu.sync() == 0
        np.testing.assert_array_equal(gpu.state_digest(), before)
        gpu.close()
    gpu = context(fa, AS.named("groups3"))
    assert lib.fpx_acceptor_inbox_dev(gpu._h, 4, p, p, p, p, p, p, 2, p, p) == EINVAL       # a grid is one group
    assert lib.fpx_acceptor_inbox(gpu._h, 4, h, h, h, h, h, h, 2, h, h) == EINVAL
    for k in (0, 2, 3, 4, 5):                                                               # group_index alone may be NULL
        args = [None if j == k else p for j in range(6)]
        assert lib.fpx_acceptor_inbox_dev(gpu._h, 4, *args, 0, p, p) == EINVAL
        assert lib.fpx_acceptor_inbox(gpu._h, 4, *[None if a is None else h for a in args], 0, h, h) == EINVAL
    for n, cols in ((-1, 0), (1 << 30, 0), (4, -1)):
        assert lib.fpx_acceptor_inbox_dev(gpu._h, n, p, p, p, p, p, p, cols, p, p) == EINVAL
        assert lib.fpx_acceptor_inbox(gpu._h, n, h, h, h, h, h, h, cols, h, h) == EINVAL
    assert lib.fpx_acceptor_inbox_dev(gpu._h, 0, *[None] * 6, 0, None, None) == 0
    assert lib.fpx_acceptor_inbox(gpu._h, 0, *[None] * 6, 0, None, None) == 0
    assert gpu.sync() == 0
    gpu.close()


@pytest.mark.parametrize("dev", [False, True])
def test_null_outputs(fa, dev):
    b = AS.named("groups3")
    gpu, twin, model = context(fa, b), context(fa, b), M.Sequential(b.R, b.groups, b.S)
    assert call(gpu, b, dev, replies=False) == (0, None, None)
    one_by_one(twin, b)
    model.run(b)
    assert_same_contexts(gpu, twin, "no outputs")
    assert_equals_model(gpu, model, "no outputs")
    # one output only
    f = AS.follow_up("groups3")
    kind, acc, slot, rnd, value, group = f.arrays()
    want = model.run(f)
    rk = np.full(len(f), -9, np.int32)
    assert fa.lib().fpx_acceptor_inbox(gpu._h, len(f), *(a.ctypes.data for a in (kind, group, acc, slot, rnd, value)), 0,
                                       rk.ctypes.data, None) == 0
    np.testing.assert_array_equal(rk, want[2])
    gpu.close(), twin.close()


def test_a_torch_stream_other_than_the_default(fa):
    import torch

    b = AS.named("R64")
    gpu, model = context(fa, b), M.Sequential(b.R, b.groups, b.S)
    side = torch.cuda.Stream()
    gpu.set_stream(side.cuda_stream)
    with torch.cuda.stream(side):
        for burst in (b, AS.follow_up("R64")):
            st, bad, want_kind, want_value = model.run(burst)
            st, rk, rv = call(gpu, burst, True)
            assert st == 0
            np.testing.assert_array_equal(rk, want_kind)
            np.testing.assert_array_equal(rv, want_value)
    assert_equals_model(gpu, model, "side stream")
    gpu.close()


def test_the_scratch_is_counted_and_kept(fa):
    b = AS.named("n3000")
    gpu = context(fa, b)
    before = gpu.device_bytes
    assert call(gpu, b, False)[0] == 0
    after = gpu.device_bytes
    assert after - before >= 12 * 8192 + 24 * 3000                     # the claim table of 2^13 words and the call's scratch
    assert call(gpu, AS.follow_up("n3000"), True)[0] == 0
    assert gpu.device_bytes == after                                   # nothing new for a burst that fits
    gpu.close()


def test_the_jni_native_on_the_mock_jvm(fa, jvm):  # noqa: F811
    b = AS.named("groups3")
    cfg = np.array([b.S, b.R, b.groups, 1, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0], np.int32)   # the 15 fpx_config fields
    h = jvm.call("create", C.c_int64, jvm.arr(cfg))
    assert h > 0
    gpu = context(fa, b)

    def native(burst, short=None, outputs=True):
        n = len(burst)
        kind, acc, slot, rnd, value, group = burst.arrays()
        arrs = [kind, group, acc, slot, rnd, value, np.full(n, -9, np.int32), np.full(n, -9, np.int32)]
        if short is not None:
            arrs[short] = arrs[short][:-1]
        handles = [jvm.arr(a) for a in arrs]
        if not outputs:
            handles[6] = handles[7] = None
        st = jvm.call("acceptorInbox", C.c_int32, h, n, *handles[:6], burst.grid_cols, *handles[6:])
        return st, [jvm.read(a, np.int32, len(arrs[6 + j])) for j, a in enumerate(handles[6:]) if a is not None]

    for burst in (b, AS.follow_up("groups3")):
        st, (rk, rv) = native(burst)
        want = call(gpu, burst, False)
        assert st == want[0] == 0
        np.testing.assert_array_equal(rk, want[1])
        np.testing.assert_array_equal(rv, want[2])
    for short in range(8):                                             # a short array is refused before native code runs
        assert native(b.cut(0, 50), short)[0] == EINVAL
    what, c, at = AS.spoiled(b)[1]                                     # a bad slot: the arrays are left as they were
    st, outs = native(c)
    assert st == EINVAL and all((o == -9).all() for o in outs)
    assert native(b.cut(0, 50), outputs=False)[0] == 0 and call(gpu, b.cut(0, 50), False, replies=False)[0] == 0
    assert jvm.call("destroy", C.c_int32, h) == 0
    gpu.close()


def test_a_gpu_acceptor_shaped_walk_on_wire_bytes(fa):
    """AcceptorInbound bytes -> fpx_wire_decode_acceptor_inbound -> the inbox -> ProxyLeaderInbound{Phase2b} /
    LeaderInbound{Nack} bytes by the existing encoders, as jni/Native.scala's GpuAcceptor walks a burst"""
    cid = bytes.fromhex("0a0d") + b"10.0.0.1:9000" + bytes.fromhex("1003" "1811")          # CommandId{address, pseudonym 3, id 17}
    max_slot = bytes([0x1a, len(cid) + 2, 0x0a, len(cid)]) + cid                             # {max_slot_request = 3}
    batch_max_slot = bytes.fromhex("22" "04" "0805" "1007")                                 # {batch_max_slot_request = 4 {5, 7}}
    cmd = bytes.fromhex("0a00")
    # (bytes, acceptor it was delivered to)
    msgs = [(wire.encode_acceptor_phase2a(5, 2, cmd), 1), (wire.encode_acceptor_phase2a(5, 2, cmd), 2),
            (max_slot, 1), (wire.encode_acceptor_phase1a(4, 0), 1), (wire.encode_acceptor_phase2a(6, 2, None), 1),
            (wire.encode_acceptor_phase2a(6, 2, None), 0), (batch_max_slot, 0), (wire.encode_acceptor_phase2a(9, 4, cmd), 1),
            (batch_max_slot, 1)]
    assert msgs[0][0].hex() == "1208080510021a020a00" and msgs[3][0].hex() == "0a0408041000"
    d = wire.decode_acceptor_inbound([m for m, _ in msgs])
    assert d["status"] == 0 and d["kind"].tolist() == [P2A, P2A, MSR, P1A, P2A, P2A, BMSR, P2A, BMSR]
    acc = np.array([a for _, a in msgs], np.int32)
    value = np.where(d["kind"] == P2A, np.where(d["is_noop"] == 1, -1, np.arange(len(msgs))), -1).astype(np.int32)
    b = AS.Burst(3, 1, 64, 0, d["kind"], np.zeros(len(msgs), np.int32), acc, d["slot"], d["round"], value)
    gpu = context(fa, b)
    st, rk, rv = call(gpu, b, False)
    assert st == 0
    assert rk.tolist() == [M.PHASE2B, M.PHASE2B, MSR, M.PHASE1B, M.NACK, M.PHASE2B, MSR, M.PHASE2B, MSR]
    assert rv.tolist() == [2, 2, 5, 4, 4, 2, 6, 4, 9]
    out = []
    for i in range(len(msgs)):
        if rk[i] == M.PHASE2B:
            out.append(wire.encode_proxy_leader_phase2b(0, int(acc[i]), int(d["slot"][i]), int(rv[i])))
        elif rk[i] == M.NACK:
            out.append((fa.round_leader(2, int(d["round"][i])), wire.encode_leader_nack(int(rv[i]))))
        elif rk[i] == MSR and d["kind"][i] == MSR:
            command_id = bytes(d["buf"][d["value_off"][i]:d["value_off"][i] + d["value_len"][i]])
            out.append(wire.encode_client_max_slot_reply(command_id, 0, int(acc[i]), int(rv[i])))
        elif rk[i] == MSR:
            out.append(wire.encode_read_batcher_batch_max_slot_reply(int(d["slot"][i]), int(d["round"][i]), int(acc[i]), int(rv[i])))
    assert out[0].hex() == "12080800100118052002"                     # Phase2b(group 0, acceptor 1, slot 5, round 2)
    assert out[3] == (0, bytes.fromhex("32020804"))                    # Nack(4) to the leader of round 2
    assert out[2] == bytes([0x22, len(cid) + 2 + 6]) + bytes([0x0a, len(cid)]) + cid + bytes.fromhex("1000" "1801" "2005")
    assert out[5] == bytes.fromhex("22" "08" "0805" "1007" "1800" "2006")
    assert len(out) == 8
    gpu.close()
