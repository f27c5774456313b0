"""The wire adapter's DEVICE encoders (include/fpx_wire.h, fpx_wire_encode_*_dev): the records of a tick in HBM -> the
serialised Chosen / Phase2b / Nack messages, back to back, with offsets and totals.  The expected bytes are the host
encoders' (one emitter source, compared whole) and the google.protobuf vectors of tests/golden/wire_vectors.json.

Record counts go around every boundary of the kernel shape: a wavefront (64), a workgroup (256 records), the single
scanning workgroup's tile (1024 workgroup sums = 2^18 records), and 2^20.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31 - 1]
ECAPACITY, EINVAL = 5, 1


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


def context(fa, **kw):
    """a context whose work is enqueued on torch's current stream: the tensors these tests fill and upload with torch are
    then ordered with the library's kernels (the context's own stream is non-blocking)"""
    import torch

    gpu = fa.Context(fa.make_config(**kw))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    return gpu


@pytest.fixture(scope="module")
def gpu(fa):
    return context(fa, num_slots=1024, num_replicas=3, f=1)


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "wire_vectors.json")))["vectors"]


def dev():
    import torch

    return torch.device("cuda:0")


def up(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev())


def host_chosen(wire, slot, is_noop, values, voff, vlen, emit=None):
    """the host encoder, one record at a time: (bytes, offsets)"""
    L = wire._L()
    out = np.zeros(int(np.maximum(vlen, 0).sum()) + 32 * len(slot) + 64, np.uint8)
    off = [0]
    at = 0
    for i in range(len(slot)):
        if emit is not None and not emit[i]:
            continue
        k = L.fpx_wire_encode_replica_chosen(out.ctypes.data + at, len(out) - at, int(slot[i]), values.ctypes.data + int(voff[i]),
                                             int(vlen[i]), int(is_noop[i]) if is_noop is not None else 0)
        assert k > 0
        at += k
        off.append(at)
    return out[:at].tobytes(), np.array(off, np.int64)


def np_chosen(slot, values, voff, L):
    """a vectorised restatement for big ticks: every record emitted, non-negative slots, one value length L < 128"""
    slot = slot.astype(np.int64)
    k = np.ones(len(slot), np.int64)
    for b in (7, 14, 21, 28):
        k += slot >= (1 << b)
    length = 2 + 1 + k + 2 + L
    assert 1 + int(k.max()) + 2 + L < 128
    off = np.zeros(len(slot) + 1, np.int64)
    np.cumsum(length, out=off[1:])
    out = np.zeros(int(off[-1]), np.uint8)
    for kk in range(1, 6):
        idx = np.nonzero(k == kk)[0]
        if not len(idx):
            continue
        rows = np.zeros((len(idx), 5 + kk + L), np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2] = 0x0a, 1 + kk + 2 + L, 0x08
        s = slot[idx]
        for j in range(kk):
            rows[:, 3 + j] = ((s >> (7 * j)) & 0x7f) | (0x80 if j < kk - 1 else 0)
        rows[:, 3 + kk], rows[:, 4 + kk] = 0x12, L
        rows[:, 5 + kk:] = values[voff[idx][:, None] + np.arange(L)[None, :]]
        out[off[idx][:, None] + np.arange(5 + kk + L)[None, :]] = rows
    return out.tobytes(), off


def chosen_case(gpu, wire, slot, is_noop, values, voff, vlen, emit=None, expect=None):
    import torch

    n = len(slot)
    cap = int(np.maximum(vlen, 0).sum()) + 32 * n + 64
    out = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device=dev())
    offs = torch.full((n + 1,), -7, dtype=torch.int64, device=dev())
    _, _, tot = gpu.wire_encode_chosen_dev(up(slot.astype(np.int32)), up(voff.astype(np.int64)), up(vlen.astype(np.int32)),
                                           up(values), emit=None if emit is None else up(emit.astype(np.uint8)),
                                           is_noop=None if is_noop is None else up(is_noop.astype(np.int32)), cap=cap,
                                           out=out, out_offsets=offs)
    assert gpu.sync() == 0
    want, woff = expect if expect is not None else host_chosen(wire, slot, is_noop, values, voff, vlen, emit)
    count, total = (int(x) for x in tot.cpu().numpy())
    assert count == len(woff) - 1 and total == len(want)
    o = out.cpu().numpy()
    assert o[:total].tobytes() == want
    assert (o[total:] == 0xC3).all()
    assert (offs.cpu().numpy()[:count + 1] == woff).all()
    return want, woff


def test_golden_chosen_through_the_device_decoder(gpu, wire, vectors):
    p2a = [v for v in vectors if v["msg"] == "phase2a"]
    msgs = [bytes.fromhex(v["proxy_leader_inbound"]) for v in p2a]
    buf, off = wire.pack(msgs)
    d = gpu.wire_decode_dev("proxy_leader_inbound", up(buf), up(off), buf_len=int(off[-1]))
    out, offs, tot = gpu.wire_encode_chosen_dev(d["slot"], d["value_off"], d["value_len"], up(buf), is_noop=d["is_noop"],
                                                values_len=int(off[-1]))
    assert gpu.sync() == 0
    want = [bytes.fromhex(v["replica_inbound_chosen"]) for v in p2a]
    count, total = (int(x) for x in tot.cpu().numpy())
    assert count == len(want) and total == sum(len(w) for w in want)
    assert out.cpu().numpy()[:total].tobytes() == b"".join(want)
    assert offs.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    # the Mencius vectors: the same Chosen message, decoded from Mencius bytes by the host decoder
    m2a = [v for v in vectors if v["msg"] == "mencius_phase2a"]
    msgs = [bytes.fromhex(v["proxy_leader_inbound"]) for v in m2a]
    h = wire.mencius_decode_proxy_leader_inbound(msgs)
    want, _ = chosen_case(gpu, wire, h["slot"], h["is_noop"], h["buf"], h["value_off"], h["value_len"])
    assert want == b"".join(bytes.fromhex(v["replica_inbound_chosen"]) for v in m2a)


def run_p2b(gpu, slot, round_, bits, gos=None, cols=0, dialect=0, cap=None, max_msgs=None):
    import torch

    n = len(slot)
    msgs = int(sum(bin(int(x)).count("1") for x in bits.reshape(-1)))
    max_msgs = msgs if max_msgs is None else max_msgs
    cap = 46 * msgs + 16 if cap is None else cap
    out = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device=dev())
    offs = torch.full((max_msgs + 1,), -7, dtype=torch.int64, device=dev())
    _, _, tot = gpu.wire_encode_phase2b_batch_dev(up(slot.astype(np.int32)), up(round_.astype(np.int32)),
                                                  up(bits.astype(np.uint64).reshape(-1)) if n else up(np.zeros(4, np.uint64)),
                                                  None if gos is None else up(gos.astype(np.int32)), cols, dialect, cap=cap,
                                                  max_msgs=max_msgs, out=out, out_offsets=offs)
    return gpu.sync(), out.cpu().numpy(), offs.cpu().numpy(), [int(x) for x in tot.cpu().numpy()]


def host_p2b(wire, slot, round_, bits, gos, cols, dialect):
    if dialect == 0:
        return wire.encode_phase2b_batch(slot, round_, bits.reshape(-1), gos, cols)
    out = []
    for i in range(len(slot)):
        for b in range(256):
            if int(bits[i][b >> 6]) >> (b & 63) & 1:
                out.append(wire.mencius_encode("proxy_leader_phase2b", b % cols if cols > 0 else b, int(slot[i]), int(round_[i])))
    return out


def p2b_case(gpu, wire, slot, round_, bits, gos=None, cols=0, dialect=0):
    want = host_p2b(wire, slot, round_, bits, gos, cols, dialect)
    st, o, offs, (count, total) = run_p2b(gpu, slot, round_, bits, gos, cols, dialect)
    assert st == 0
    assert count == len(want) and total == sum(len(w) for w in want)
    assert o[:total].tobytes() == b"".join(want)
    assert (o[total:] == 0xC3).all()
    assert offs[:count + 1].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want], dtype=np.int64)]).astype(np.int64).tolist()


def bit_rows(rows):
    out = np.zeros((len(rows), 4), np.uint64)
    for i, r in enumerate(rows):
        for b in r:
            out[i][b >> 6] |= np.uint64(1 << (b & 63))
    return out


def test_golden_phase2b_and_nack_both_dialects(gpu, wire, vectors):
    p2b = [v for v in vectors if v["msg"] == "phase2b"]
    # every vector is one bit of one row: bit = acceptor_index, the group comes in as group_of_slot
    slot = np.array([v["slot"] for v in p2b], np.int32)
    round_ = np.array([v["round"] for v in p2b], np.int32)
    ok = [i for i, v in enumerate(p2b) if 0 <= v["acceptor_index"] < 256]
    assert ok
    bits = bit_rows([[p2b[i]["acceptor_index"]] for i in ok])
    gos = np.array([p2b[i]["group_index"] for i in ok], np.int32)
    st, o, offs, (count, total) = run_p2b(gpu, slot[ok], round_[ok], bits, gos)
    assert st == 0 and count == len(ok)
    assert o[:total].tobytes() == b"".join(bytes.fromhex(p2b[i]["proxy_leader_inbound"]) for i in ok)
    rng = [v for v in vectors if v["msg"] == "mencius_ranges" and 0 <= v["acceptor"] < 256]
    assert rng
    st, o, offs, (count, total) = run_p2b(gpu, np.array([v["start"] for v in rng]), np.array([v["round"] for v in rng]),
                                          bit_rows([[v["acceptor"]] for v in rng]), dialect=1)
    assert st == 0 and count == len(rng)
    assert o[:total].tobytes() == b"".join(bytes.fromhex(v["pl_phase2b"]) for v in rng)
    for dialect, vs, key in ((0, [v for v in vectors if v["msg"] == "phase1a_nack"], "leader_inbound_nack"), (1, rng, "leader_nack")):
        rounds = np.array([v["round"] for v in vs], np.int32)
        keep = rounds >= 0
        out, offs, tot = gpu.wire_encode_leader_nack_dev(up(rounds), dialect)
        assert gpu.sync() == 0
        want = [bytes.fromhex(v[key]) for v, k in zip(vs, keep) if k]
        count, total = (int(x) for x in tot.cpu().numpy())
        assert count == len(want) and out.cpu().numpy()[:total].tobytes() == b"".join(want)
        assert offs.cpu().numpy()[:count + 1].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()


def random_chosen_tick(rng, n, lens, noop_share=0.2):
    """values at every alignment mod 16: each value starts a random 0..15 bytes after the one before"""
    vlen = rng.choice(lens, n).astype(np.int32)
    gap = rng.integers(0, 16, n)
    voff = np.cumsum(gap + np.concatenate([[0], vlen[:-1]])).astype(np.int64)
    values = rng.integers(0, 256, int(voff[-1] + vlen[-1]) + 16 if n else 16, dtype=np.uint8)
    slot = rng.choice(EDGES + [5, 300, 70000], n).astype(np.int32)
    is_noop = (rng.random(n) < noop_share).astype(np.int32)
    return slot, is_noop, values, voff, vlen


@pytest.mark.parametrize("mask", ["none", "all", "random"])
def test_random_chosen_ticks_equal_the_host_encoder(gpu, wire, mask):
    rng = np.random.default_rng(11)
    for n, lens in ((700, [0, 1, 127, 128, 300]), (130, [0, 1, 127, 128, 300, 20000]), (64, [20000]), (16, [1])):
        slot, is_noop, values, voff, vlen = random_chosen_tick(rng, n, lens)
        assert set((voff % 16).tolist()) == set(range(16)) or n < 100
        emit = {"none": np.zeros(n, np.uint8), "all": None, "random": (rng.random(n) < 0.5).astype(np.uint8)}[mask]
        chosen_case(gpu, wire, slot, is_noop, values, voff, vlen, emit)
    # a negative value_len counts as 0, as in the host encoder; negative slots are ten-byte varints
    slot, is_noop, values, voff, vlen = random_chosen_tick(rng, 90, [3, 40], 0.0)
    vlen[::7] = -5
    slot[::5] = -1
    chosen_case(gpu, wire, slot, None, values, voff, vlen)


def test_random_vote_rows_equal_the_host_encoder(gpu, wire):
    rng = np.random.default_rng(12)
    def rows(n):
        out = []
        for i in range(n):
            k = i % 5
            out.append([] if k == 0 else [int(rng.integers(0, 256))] if k == 1 else
                       sorted(rng.choice(255, 127, replace=False).tolist()) if k == 2 else list(range(256)) if k == 3 else
                       sorted(rng.choice(256, int(rng.integers(1, 9)), replace=False).tolist()))
        return bit_rows(out)
    for n in (1, 7, 70, 300):
        slot = rng.choice(EDGES, n).astype(np.int32)
        round_ = rng.choice(EDGES, n).astype(np.int32)
        gos = rng.choice([0, 1, 127, 128, 300], n).astype(np.int32)
        for cols, g, dialect in ((0, None, 0), (0, gos, 0), (16, None, 0), (1, None, 0), (200, gos, 0), (255, None, 0), (300, None, 0),
                                 (0, None, 1), (16, None, 1), (200, None, 1)):
            p2b_case(gpu, wire, slot, round_, rows(n), g, cols, dialect)
    # R = 1 ... a full row, one record each
    for r in (1, 2, 3, 64, 65, 128, 129, 255, 256):
        p2b_case(gpu, wire, np.array([r]), np.array([2]), bit_rows([list(range(r))]))


COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, (1 << 16) + 3, (1 << 18) - 1, (1 << 18) + 257, 1 << 20]


@pytest.mark.parametrize("n", COUNTS)
def test_chosen_record_counts_around_the_kernel_shape(gpu, wire, n):
    rng = np.random.default_rng(n)
    L = 16
    slot = ((np.arange(n, dtype=np.int64) * 2053 + int(rng.integers(0, 1 << 20))) % (1 << 31)).astype(np.int32)
    voff = (np.arange(n, dtype=np.int64) * 17 + 3)          # every alignment mod 16
    values = rng.integers(0, 256, int(voff[-1]) + L + 16, dtype=np.uint8)
    vlen = np.full(n, L, np.int32)
    restated = np_chosen(slot, values, voff, L)
    if n <= 1025:  # the restatement itself is held against the host encoder where that is cheap
        h = host_chosen(wire, slot, None, values, voff, vlen)
        assert h[0] == restated[0] and (h[1] == restated[1]).all()
    chosen_case(gpu, wire, slot, None, values, voff, vlen, expect=restated)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, (1 << 16) + 3, 1 << 20])
def test_phase2b_and_nack_record_counts_around_the_kernel_shape(gpu, wire, n):
    rng = np.random.default_rng(n)
    slot = rng.integers(0, 1 << 22, n).astype(np.int32)
    round_ = rng.integers(0, 300, n).astype(np.int32)
    bits = np.zeros((n, 4), np.uint64)
    bits[:, 0] = rng.integers(0, 8, n).astype(np.uint64)   # R = 3: any subset of three acceptors
    want_bytes = np.zeros(n * 3 * 16 + 16, np.uint8)
    want_off = np.zeros(n * 3 + 1, np.int64)
    k = wire._L().fpx_wire_encode_phase2b_batch(n, slot.ctypes.data, round_.ctypes.data, bits.ctypes.data, None, 0,
                                                want_bytes.ctypes.data, len(want_bytes), want_off.ctypes.data, n * 3)
    assert k >= 0
    st, o, offs, (count, total) = run_p2b(gpu, slot, round_, bits)
    assert st == 0 and count == k and total == want_off[k]
    assert (o[:total] == want_bytes[:total]).all() and (offs[:k + 1] == want_off[:k + 1]).all()
    # Nack rounds: -1 = none
    nack = np.where(rng.random(n) < 0.5, -1, rng.choice(EDGES, n)).astype(np.int32)
    out, offs, tot = gpu.wire_encode_leader_nack_dev(up(nack))
    assert gpu.sync() == 0
    r = nack[nack >= 0].astype(np.int64)
    kk = np.ones(len(r), np.int64)
    for b in (7, 14, 21, 28):
        kk += r >= (1 << b)
    woff = np.concatenate([[0], np.cumsum(3 + kk)])
    count, total = (int(x) for x in tot.cpu().numpy())
    assert count == len(r) and total == woff[-1] and (offs.cpu().numpy()[:count + 1] == woff).all()
    o = out.cpu().numpy()
    pick = rng.integers(0, max(1, len(r)), 200) if len(r) else []
    for j in pick:  # the host encoder on a sample; the lengths of all
        assert o[woff[j]:woff[j + 1]].tobytes() == wire.encode_leader_nack(int(r[j]))
    if n <= 1025:
        assert o[:total].tobytes() == b"".join(wire.encode_leader_nack(int(x)) for x in r)


def test_capacity_is_a_per_call_code_not_an_abort(fa, wire):
    import torch

    gpu = context(fa, num_slots=1024, num_replicas=3, f=1)
    rng = np.random.default_rng(13)
    n = 300
    slot, is_noop, values, voff, vlen = random_chosen_tick(rng, n, [0, 1, 127, 128, 300])
    want, woff = host_chosen(wire, slot, is_noop, values, voff, vlen)
    args = (up(slot), up(voff), up(vlen), up(values))
    out = torch.full((len(want) + 64,), 0xC3, dtype=torch.uint8, device=dev())
    offs = torch.full((n + 1,), -7, dtype=torch.int64, device=dev())
    _, _, tot = gpu.wire_encode_chosen_dev(*args, is_noop=up(is_noop), cap=len(want) - 1, out=out, out_offsets=offs)
    # a fused step enqueued BEHIND the failed encode, before any sync, applies: the status was no abort
    s = torch.arange(64, dtype=torch.int32, device=dev())
    ch = torch.zeros(64, dtype=torch.uint8, device=dev())
    gpu.phase2_fused_dev(s, torch.zeros_like(s), s.clone(), chosen=ch)
    assert gpu.sync() == ECAPACITY
    assert bool(ch.all())
    assert tot.cpu().numpy().tolist() == [n, len(want)]
    assert bool((out == 0xC3).all()) and offs.cpu().numpy().tolist() == [0] + [-7] * n
    # the retry with the reported size
    _, _, tot = gpu.wire_encode_chosen_dev(*args, is_noop=up(is_noop), cap=len(want), out=out, out_offsets=offs)
    assert gpu.sync() == 0
    assert out.cpu().numpy()[:len(want)].tobytes() == want and (offs.cpu().numpy() == woff).all()
    # max_msgs one short (Phase2b, Nack), cap one short (Phase2b)
    sl, rd = np.arange(50, dtype=np.int32), np.full(50, 3, np.int32)
    bits = bit_rows([[0, 1, 2]] * 50)
    for kw in (dict(max_msgs=149), dict(cap=sum(len(m) for m in wire.encode_phase2b_batch(sl, rd, bits.reshape(-1))) - 1)):
        st, o, of, (count, total) = run_p2b(gpu, sl, rd, bits, **kw)
        assert st == ECAPACITY and count == 150 and (o == 0xC3).all() and of[0] == 0 and (of[1:] == -7).all()
    st, o, of, (count, total) = run_p2b(gpu, sl, rd, bits, max_msgs=150, cap=total)
    assert st == 0 and o[:total].tobytes() == b"".join(wire.encode_phase2b_batch(sl, rd, bits.reshape(-1)))
    nack = up(np.arange(40, dtype=np.int32))
    offs = torch.full((40,), -7, dtype=torch.int64, device=dev())
    _, _, tot = gpu.wire_encode_leader_nack_dev(nack, max_msgs=39, out_offsets=offs)
    assert gpu.sync() == ECAPACITY and tot.cpu().numpy().tolist() == [40, 40 * 4] and offs.cpu().numpy().tolist() == [0] + [-7] * 39
    gpu.close()


def test_bad_value_span_is_einval_with_the_index(fa, wire):
    import torch

    gpu = context(fa, num_slots=1024, num_replicas=3, f=1)
    rng = np.random.default_rng(14)
    n = 600
    slot, is_noop, values, voff, vlen = random_chosen_tick(rng, n, [1, 40], 0.0)
    for k, (i, (o, l)) in enumerate(((411, (len(values) - 3, 4)), (300, (-1, 2)), (599, (len(values) + 1, 0)))):
        vo, vl = voff.copy(), vlen.copy()
        vo[i], vl[i] = o, l
        vo[500], vl[500] = -9, 1      # a later offender (or an earlier record index wins)
        out = torch.full((70000,), 0xC3, dtype=torch.uint8, device=dev())
        offs = torch.full((n + 1,), -7, dtype=torch.int64, device=dev())
        gpu.wire_encode_chosen_dev(up(slot), up(vo), up(vl), up(values), out=out, out_offsets=offs)
        s = torch.arange(64 * k, 64 * k + 64, dtype=torch.int32, device=dev())
        ch = torch.zeros(64, dtype=torch.uint8, device=dev())
        gpu.phase2_fused_dev(s, torch.zeros_like(s), s.clone(), chosen=ch)
        assert gpu.sync() == EINVAL and gpu.error_detail()[0] == min(i, 500)
        assert bool(ch.all())           # no abort
        assert bool((out == 0xC3).all()) and offs.cpu().numpy().tolist() == [0] + [-7] * n
    # the same span on a record that is not emitted, or is a Noop, is nobody's business
    vo, vl = voff.copy(), vlen.copy()
    vo[7], vo[9] = -1, 1 << 40
    emit = np.ones(n, np.uint8)
    emit[7] = 0
    noop = np.zeros(n, np.int32)
    noop[9] = 1
    vo_h = vo.copy()
    vo_h[7] = vo_h[9] = 0
    chosen_case(gpu, wire, slot, noop, values, vo, vl, emit, expect=host_chosen(wire, slot, noop, values, vo_h, vl, emit))
    gpu.close()


def _field(num, wt, payload):
    from tests.test_wire_dev import _field as f

    return f(num, wt, payload)


@pytest.mark.parametrize("R,f", [(3, 1), (256, 127)])
def test_bytes_to_chosen_bytes_on_the_device(fa, oracle, wire, vectors, R, f):
    """decode -> fused step -> Chosen encode without the host touching a byte; the result, decoded by the host decoder,
    is the oracle's chosen (slot, value) list, every value's bytes identical to the inbound message's"""
    import torch

    S = 1 << 13
    kw = dict(num_slots=S, num_replicas=R, f=f, ballot_mode=fa.FPX_BALLOT_PER_SLOT)  # (the golden vectors' rounds differ)
    gpu, ref = context(fa, **kw), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(15)
    golden = [v for v in vectors if v["msg"] == "phase2a" and 0 <= v["slot"] < S and 0 <= v["round"] < 1000]
    assert len(golden) >= 3
    taken = {}
    for v in golden:
        taken.setdefault(v["slot"], v)
    msgs = [bytes.fromhex(v["proxy_leader_inbound"]) for v in taken.values()]
    rounds = {s: v["round"] for s, v in taken.items()}
    free = [s for s in rng.permutation(S).tolist() if s not in taken][:S // 2]
    for s in free:
        c = None if rng.random() < 0.2 else _field(1, 2, _field(1, 2, bytes(rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8))))
        msgs.append(wire.encode_proxy_leader_phase2a(int(s), 0, c))
    buf, off = wire.pack(msgs)
    n = len(msgs)
    host = wire.decode_proxy_leader_inbound(msgs)
    dbuf = up(buf)
    d = gpu.wire_decode_dev("proxy_leader_inbound", dbuf, up(off), buf_len=int(off[-1]))
    ch = torch.zeros(n, dtype=torch.uint8, device=dev())
    gpu.phase2_fused_dev(d["slot"], d["round"], d["value_id"], None, ch)
    out, offs, tot = gpu.wire_encode_chosen_dev(d["slot"], d["value_off"], d["value_len"], dbuf, emit=ch, is_noop=d["is_noop"],
                                                cap=int(off[-1]), values_len=int(off[-1]))
    assert gpu.sync() == 0
    ro = ref.phase2_fused(host["slot"], host["round"], np.arange(n, dtype=np.int32))
    assert ro[0] == 0
    chosen = np.nonzero(ro[1])[0]
    assert len(chosen) > n // 2
    count, total = (int(x) for x in tot.cpu().numpy())
    assert count == len(chosen)
    o, of = out.cpu().numpy(), offs.cpu().numpy()
    got = [o[of[k]:of[k + 1]].tobytes() for k in range(count)]
    back = wire.decode_replica_inbound(got)
    assert back["status"] == 0 and (back["kind"] == wire.CHOSEN).all()
    assert (back["slot"] == host["slot"][chosen]).all()
    all_in, all_out = b"".join(msgs), b"".join(got)
    for k, i in enumerate(chosen):
        assert bool(back["is_noop"][k]) == bool(host["is_noop"][i])
        a, b = int(back["value_off"][k]), int(host["value_off"][i])
        if not host["is_noop"][i]:
            assert all_out[a:a + int(back["value_len"][k])] == all_in[b:b + int(host["value_len"][i])]
    gpu.close()
