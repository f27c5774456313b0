"""fpx_wire_phase2_tick (include/fpx_wire.h): one proxy-leader tick bytes to bytes on page-locked buffers -- through the
ctypes binding and through the JNI native wirePhase2Tick on the mock JVM of tests/test_jni_shim.py -- against the
step-by-step path (device decode, fused step, device Chosen encode) on a second context.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)
from tests.test_wire_dev import _field

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY, EORDER = 1, 5, 6
S = 1 << 12
KW = dict(num_slots=S, num_replicas=3, f=1)


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def tick_messages(wire, rng, slots, round_=0):
    out = []
    for s in slots:
        c = None if rng.random() < 0.2 else _field(1, 2, _field(1, 2, bytes(rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8))))
        out.append(wire.encode_proxy_leader_phase2a(int(s), round_, c))
    return out


class Pinned:
    """the tick's buffers in fpx_host_alloc memory"""

    def __init__(self, fa, wire, msgs, out_cap=None):
        from frankenpaxos_amd.context import PinnedArray

        buf, off = wire.pack(msgs)
        self.n, self.in_len = len(msgs), int(off[-1])
        self.out_cap = self.in_len if out_cap is None else out_cap
        self.keep = [PinnedArray(max(1, self.in_len), np.uint8), PinnedArray(self.n + 1, np.int64),
                     PinnedArray(max(1, self.out_cap) + 16, np.uint8), PinnedArray(self.n + 1, np.int64),
                     PinnedArray(max(1, self.n), np.int32)]
        self.inb, self.ino, self.out, self.outo, self.nack = (k.array for k in self.keep)
        self.inb[:self.in_len] = buf[:self.in_len]
        self.ino[:] = off
        self.out[:] = 0xC3
        self.outo[:] = -7
        self.nack[:] = -9

    def run(self, gpu):
        return gpu.wire_phase2_tick(self.inb.ctypes.data, self.in_len, self.ino.ctypes.data, self.n, self.out.ctypes.data,
                                    self.out_cap, self.outo.ctypes.data, self.nack.ctypes.data)


def step_by_step(fa, wire, msgs, before=()):
    """the same tick on a fresh context through the three _dev calls: (chosen bytes, offsets, nack rounds, digest)"""
    import torch

    dev = torch.device("cuda:0")
    gpu = fa.Context(fa.make_config(**KW))
    # on torch's current stream: the uploads and fills below are torch's, and the context's own stream is non-blocking
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    for earlier in before + (msgs,):
        buf, off = wire.pack(earlier)
        n = len(earlier)
        dbuf = torch.from_numpy(buf).to(dev)
        d = gpu.wire_decode_dev("proxy_leader_inbound", dbuf, torch.from_numpy(off).to(dev), buf_len=int(off[-1]))
        ch = torch.zeros(n, dtype=torch.uint8, device=dev)
        nr = torch.zeros(n, dtype=torch.int32, device=dev)
        gpu.phase2_fused_dev(d["slot"], d["round"], d["value_id"], None, ch, None, None, nr)
        out, offs, tot = gpu.wire_encode_chosen_dev(d["slot"], d["value_off"], d["value_len"], dbuf, emit=ch,
                                                    is_noop=d["is_noop"], cap=int(off[-1]), values_len=int(off[-1]))
        assert gpu.sync() == 0
    count, total = (int(x) for x in tot.cpu().numpy())
    res = (out.cpu().numpy()[:total].tobytes(), offs.cpu().numpy()[:count + 1].copy(), nr.cpu().numpy().copy(), gpu.state_digest())
    gpu.close()
    return res


def test_tick_equals_the_step_by_step_path(fa, wire):
    rng = np.random.default_rng(21)
    gpu = fa.Context(fa.make_config(**KW))
    first = tick_messages(wire, rng, rng.permutation(S)[:3000], round_=1)
    # the second tick: new slots, old slots in a higher round (chosen again) and in a lower one (Nack, nothing chosen)
    second = tick_messages(wire, rng, rng.permutation(S)[:2500], round_=2)
    p1, p2 = Pinned(fa, wire, first), Pinned(fa, wire, second)
    for p, msgs, before in ((p1, first, ()), (p2, second, (first,))):
        st, count, need, bad = p.run(gpu)
        want, woff, wnack, wdig = step_by_step(fa, wire, msgs, before)
        assert st == 0 and count == len(woff) - 1 and need == len(want) and count > 0
        assert p.out[:need].tobytes() == want and (p.out[p.out_cap:] == 0xC3).all()   # (out[need .. out_cap) is unspecified)
        assert (p.outo[:count + 1] == woff).all()
        assert (p.nack == wnack).all()
        assert (gpu.state_digest() == wdig).all()
    # a third tick in a LOWER round: every message is answered by a Nack round, nothing is chosen
    third = tick_messages(wire, rng, rng.permutation(S)[:100], round_=0)
    p3 = Pinned(fa, wire, third)
    st, count, need, bad = p3.run(gpu)
    want, woff, wnack, wdig = step_by_step(fa, wire, third, (first, second))
    assert st == 0 and (p3.nack == wnack).all() and count == len(woff) - 1 and p3.out[:need].tobytes() == want
    # n == 0
    assert Pinned(fa, wire, []).run(gpu)[:2] == (0, 0)
    gpu.close()


def test_odd_encodings_never_need_more_than_the_inbound_bytes(fa, wire):
    """the documented bound: out_cap = in_len always suffices, also for encodings no encoder of ours writes (fields in any
    order, unknown fields, non-minimal varints, both members of a oneof)"""
    rng = np.random.default_rng(22)
    from tests.test_wire_dev import _varint

    def padded(v, k):  # a non-minimal varint of k bytes
        return bytes([(v >> (7 * j)) & 0x7f | 0x80 for j in range(k - 1)]) + bytes([(v >> (7 * (k - 1))) & 0x7f])

    msgs = []
    for s in rng.permutation(S)[:1500].tolist():
        cmd = _field(1, 2, _field(1, 2, bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))))
        val = [_field(2, 2, b""), cmd, _field(2, 2, b"") + cmd, cmd + _field(2, 2, b""), _field(7, 0, _varint(5)) + cmd][int(rng.integers(0, 5))]
        parts = [_varint(1 << 3) + padded(s, int(rng.integers(2, 6))), _field(2, 0, _varint(int(rng.integers(0, 1 << 20)))),
                 _varint(3 << 3 | 2) + padded(len(val), int(rng.integers(2, 5))) + val, _field(9, 0, _varint(77)),
                 _field(10, 2, bytes(int(rng.integers(0, 9))))]
        body = b"".join(parts[i] for i in rng.permutation(len(parts)))
        m = _field(1, 2, body)
        if rng.random() < 0.3:
            m = _field(1, 2, _field(1, 0, _varint(3)) + _field(2, 0, _varint(1)) + _field(3, 2, _field(2, 2, b""))) + m  # the last wins
        msgs.append(m)
    host = wire.decode_proxy_leader_inbound(msgs)
    assert host["status"] == 0 and (host["kind"] == wire.PHASE2A).all() and len(set(host["slot"].tolist())) == len(msgs)
    # rounds differ per message: a context whose ballots are per slot takes them as one run
    gpu = fa.Context(fa.make_config(ballot_mode=fa.FPX_BALLOT_PER_SLOT, **KW))
    p = Pinned(fa, wire, msgs)
    st, count, need, bad = p.run(gpu)
    assert st == 0 and count == len(msgs) and need <= p.in_len - 2 * len(msgs)
    got = [p.out[p.outo[k]:p.outo[k + 1]].tobytes() for k in range(count)]
    back = wire.decode_replica_inbound(got)
    host = wire.decode_proxy_leader_inbound(msgs)
    assert back["status"] == 0 and (back["slot"] == host["slot"]).all() and (back["is_noop"] == host["is_noop"]).all()
    gpu.close()


def test_too_small_an_out_is_ecapacity_and_the_tick_was_applied(fa, wire):
    rng = np.random.default_rng(23)
    gpu = fa.Context(fa.make_config(**KW))
    msgs = tick_messages(wire, rng, rng.permutation(S)[:500])
    want, woff, wnack, wdig = step_by_step(fa, wire, msgs)
    p = Pinned(fa, wire, msgs, out_cap=len(want) - 1)
    st, count, need, bad = p.run(gpu)
    assert st == ECAPACITY and count == 0 and need == len(want) and p.outo[0] == 0
    assert (gpu.state_digest() == wdig).all()      # applied
    assert (p.nack == wnack).all()
    gpu.close()


def test_refused_ticks_leave_the_acceptors_alone(fa, wire):
    rng = np.random.default_rng(24)
    gpu = fa.Context(fa.make_config(**KW))
    warm = tick_messages(wire, rng, range(0, 64))
    assert Pinned(fa, wire, warm).run(gpu)[0] == 0
    before = gpu.state_digest()
    msgs = tick_messages(wire, rng, range(100, 400))
    # pageable memory
    buf, off = wire.pack(msgs)
    out, outo = np.zeros(len(buf), np.uint8), np.zeros(len(msgs) + 1, np.int64)
    st = gpu.wire_phase2_tick(buf.ctypes.data, int(off[-1]), off.ctypes.data, len(msgs), out.ctypes.data, len(out),
                              outo.ctypes.data)[0]
    assert st == EINVAL and (gpu.state_digest() == before).all()
    # a Phase2b in the tick
    bad = list(msgs)
    bad[37] = wire.encode_proxy_leader_phase2b(0, 1, 5, 0)
    st, count, need, idx = Pinned(fa, wire, bad).run(gpu)
    assert st == EINVAL and idx == 37 and count == 0 and (gpu.state_digest() == before).all()
    # a malformed message
    bad = list(msgs)
    bad[211] = bad[211][:-1]
    st, count, need, idx = Pinned(fa, wire, bad).run(gpu)
    assert st == EINVAL and idx == 211 and (gpu.state_digest() == before).all()
    # a slot outside the window
    bad = list(msgs)
    bad[5] = wire.encode_proxy_leader_phase2a(S + 3, 0, None)
    st, count, need, idx = Pinned(fa, wire, bad).run(gpu)
    assert st == EINVAL and idx == 5 and (gpu.state_digest() == before).all()
    # not one device run: the same slot twice
    bad = list(msgs)
    bad[150] = bad[20]
    st, count, need, idx = Pinned(fa, wire, bad).run(gpu)
    assert st == EORDER and count == 0 and (gpu.state_digest() == before).all()
    # ... and the context goes on
    p = Pinned(fa, wire, msgs)
    st, count, need, idx = p.run(gpu)
    assert st == 0 and count == len(msgs)
    gpu.close()


def test_the_jni_native_walks_the_same_tick(fa, wire, jvm):  # noqa: F811
    rng = np.random.default_rng(25)
    msgs = tick_messages(wire, rng, rng.permutation(S)[:700])
    want, woff, wnack, wdig = step_by_step(fa, wire, msgs)
    buf, off = wire.pack(msgs)
    n, in_len = len(msgs), int(off[-1])
    gpu = fa.Context(fa.make_config(**KW))
    h = gpu._h.value if hasattr(gpu._h, "value") else int(gpu._h)

    def direct(nbytes, fill=None):
        d = C.c_void_p(jvm.call("hostAlloc", C.c_void_p, C.c_int64(max(1, nbytes))))
        assert d.value
        if fill is not None:
            C.memmove(jvm.lib.mock_data(d), fill.ctypes.data, fill.nbytes)
        return d

    din, dino = direct(in_len, buf[:in_len]), direct(8 * (n + 1), off)
    dout, douto, dnack = direct(in_len), direct(8 * (n + 1)), direct(4 * n)
    counts = jvm.arr(np.zeros(3, np.int64))
    call = lambda *a: jvm.call("wirePhase2Tick", C.c_int32, C.c_int64(h), *a)
    # the array-length checks every native has: short buffers and a short counts array are refused before anything runs
    assert call(din, C.c_int64(in_len + 1), dino, n, dout, douto, dnack, counts) == EINVAL
    assert call(din, C.c_int64(in_len), direct(8 * n), n, dout, douto, dnack, counts) == EINVAL
    assert call(din, C.c_int64(in_len), dino, n, dout, direct(8 * n), dnack, counts) == EINVAL
    assert call(din, C.c_int64(in_len), dino, n, dout, douto, direct(4 * n - 1), counts) == EINVAL
    assert call(din, C.c_int64(in_len), dino, n, dout, douto, dnack, jvm.arr(np.zeros(2, np.int64))) == EINVAL
    assert call(din, C.c_int64(in_len), dino, n, jvm.arr(np.zeros(in_len, np.int8)), douto, dnack, counts) == EINVAL  # not direct
    assert call(din, C.c_int64(in_len), dino, n, dout, douto, dnack, counts) == 0
    count, need, bad = jvm.read(counts, np.int64, 3)
    assert count == len(woff) - 1 and need == len(want) and bad == -1
    raw = lambda d, dtype, k: np.ctypeslib.as_array(C.cast(jvm.lib.mock_data(d), C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (k,)).copy()
    assert raw(dout, np.uint8, need).tobytes() == want
    assert (raw(douto, np.int64, count + 1) == woff).all() and (raw(dnack, np.int32, n) == wnack).all()
    assert (gpu.state_digest() == wdig).all()
    gpu.close()
