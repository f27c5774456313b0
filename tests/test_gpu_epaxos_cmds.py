"""The EPaxos context's command store (fpx_epx_cmds_*, csrc/fpx_epx_cmds.hpp) against a Python dict in which the first
stored wins: cmds_read of every id, and the arena as a whole, which must be the concatenation of the writers' commands in
index order -- at every length at which the copy takes another path, every source alignment and arena fill position mod 16,
bursts at the wavefront, workgroup and scan-row edges, in both copy forms; the skips, the refused burst, the bad span; result
and cmds_stats asserted exactly."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EINVAL = 1
MAX_LEN = 1 << 16
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 100, 101, 4097, MAX_LEN)


def make(max_triples, arena_bytes, bytewise=False):
    """a context with the store, in the copy form named (FPX_EPX_CMDS_WORDS is read by fpx_epx_create; the single-byte form is
    the default)"""
    from frankenpaxos_amd.epaxos import EPaxos

    old = os.environ.pop("FPX_EPX_CMDS_WORDS", None)
    if not bytewise:
        os.environ["FPX_EPX_CMDS_WORDS"] = "1"
    e = EPaxos(3, 4, num_instances=8)
    os.environ.pop("FPX_EPX_CMDS_WORDS", None)
    if old is not None:
        os.environ["FPX_EPX_CMDS_WORDS"] = old
    e.cmds_enable(max_triples, arena_bytes)
    return e


@pytest.fixture(scope="module", params=["words", "bytes"])
def form(request):
    return request.param == "bytes"


def blob(length, salt):
    return (np.arange(length, dtype=np.int64) * 131 + salt * 7 + (np.arange(length, dtype=np.int64) >> 7)).astype(np.uint8).tobytes()


class Model:
    """the store as a dict, with the arena and the four counts"""

    def __init__(self, max_triples, arena_bytes):
        self.max_triples, self.arena_bytes = max_triples, arena_bytes
        self.cmds, self.arena, self.skipped, self.refused = {}, b"", 0, 0

    def put(self, commands, ids):
        """-> result[4]"""
        fresh, skipped, seen = [], 0, set()
        for c, t in zip(commands, ids):
            if t < 0 or c is None:
                continue
            if t >= self.max_triples or len(c) > MAX_LEN:
                skipped += 1
            elif t not in self.cmds and t not in seen:
                seen.add(t)
                fresh.append((t, c))
        self.skipped += skipped
        new = sum(len(c) for _, c in fresh)
        if len(self.arena) + new > self.arena_bytes:
            self.refused += 1
            return [0, 0, skipped, 1]
        for t, c in fresh:
            self.cmds[t] = c
            self.arena += c
        return [len(fresh), new, skipped, 0]

    def stats(self):
        return (len(self.cmds), len(self.arena), self.skipped, self.refused)


def pack(commands, lead=0, gap=0):
    """the commands in one buffer, the first `lead` bytes behind its start and `gap` bytes between neighbours; a None is a
    record without a command (-1, -1): (buf, off, len)"""
    buf, off, ln = bytearray(b"\xAA" * lead), [], []
    for c in commands:
        if c is None:
            off.append(-1), ln.append(-1)
            continue
        off.append(len(buf)), ln.append(len(c))
        buf += c + b"\xAA" * gap
    return np.frombuffer(bytes(buf) or b"\0", np.uint8), np.array(off, np.int64), np.array(ln, np.int32)


def check(e, model, ids_to_read):
    assert e.cmds_stats() == model.stats()
    for t in ids_to_read:
        assert e.cmds_read(t) == model.cmds.get(t), t


def arena_of(e, model):
    """the arena as a whole, read through the ids in the order of their offsets: the model's concatenation"""
    return b"".join(e.cmds_read(t) for t in model.cmds)       # (a dict keeps insertion order: the writers' index order)


def put(e, model, commands, ids, **kw):
    st, res = e.cmds_put(packed=pack(commands, **kw), triple_id=ids)
    assert st == 0 and list(res) == model.put(commands, ids)


@pytest.mark.parametrize("lead", range(16))
def test_every_length_at_every_source_alignment_and_fill_position(form, lead):
    """a first put of `lead` bytes moves the arena's fill position; the source starts `lead` bytes behind a 16-byte
    boundary and the odd gaps walk every source alignment against every destination alignment"""
    cap = lead + sum(LENGTHS) + 64
    e, model = make(64, cap, form), Model(64, cap)
    try:
        put(e, model, [blob(lead, 99)], [40])
        commands = [blob(n, k) for k, n in enumerate(LENGTHS)] + [blob(MAX_LEN + 1, 5)]
        ids = list(range(len(LENGTHS))) + [20]
        put(e, model, commands, ids, lead=lead, gap=lead % 3 + (lead & 1))
        assert model.skipped == 1 and 20 not in model.cmds and len(model.cmds) == len(LENGTHS) + 1
        check(e, model, list(range(24)) + [40])
        assert arena_of(e, model) == model.arena
    finally:
        e.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_bursts_at_the_wavefront_workgroup_and_row_edges(form, m):
    rng = np.random.default_rng(m)
    max_triples = m + 8
    lens = rng.choice([0, 1, 3, 15, 16, 17, 40, 63, 64, 65, 100, 101, 300], size=m)
    commands = [blob(int(n), j) for j, n in enumerate(lens)]
    ids = list(rng.permutation(m).astype(int))
    # one id three times with different bytes (the lowest index wins), records without a command, ids -1 and max_triples
    if m >= 63:
        for j in (5, 30, 61):
            ids[j] = m + 1
        commands[17], ids[17] = None, -1
        ids[18], ids[19] = -1, max_triples
        ids[m - 1] = m + 2
    cap = sum(len(c) for c in commands if c is not None) + 5000
    e, model = make(max_triples, cap, form), Model(max_triples, cap)
    try:
        put(e, model, commands, ids, lead=m % 16, gap=m % 5)
        if m >= 63:
            assert model.cmds[m + 1] == commands[5] and model.skipped == 1
        # a second burst: ids already present keep their bytes, new ids land behind
        again = [blob(33 + j % 7, 1000 + j) for j in range(min(m, 70))]
        ids2 = [ids[0]] + [m + 3 + j % 5 for j in range(len(again) - 1)]
        put(e, model, again, ids2)
        assert model.cmds[ids[0]] == commands[0]
        check(e, model, range(max_triples))
        assert arena_of(e, model) == model.arena
    finally:
        e.close()


def test_a_burst_one_byte_too_large_stores_nothing_and_the_next_lands_there(form):
    first, big = blob(7, 1), [blob(100, 2), blob(29, 3)]
    cap = len(first) + 128
    e, model = make(16, cap, form), Model(16, cap)
    try:
        put(e, model, [first], [0])
        st, res = e.cmds_put(big, [1, 2])                      # 129 new bytes into 128 free
        assert st == 0 and list(res) == model.put(big, [1, 2]) == [0, 0, 0, 1]
        check(e, model, range(16))
        assert e.sync() == 0                                   # no context status
        put(e, model, [blob(100, 4), blob(28, 5)], [2, 1])     # 128: exactly the free arena, where the refused one would be
        assert model.stats() == (3, cap, 0, 1)
        check(e, model, range(16))
        assert arena_of(e, model) == model.arena and e.cmds_read(2) == blob(100, 4)
        st, res = e.cmds_put([b"x"], [3])                      # a full arena refuses one byte, and takes none
        assert st == 0 and list(res) == model.put([b"x"], [3]) == [0, 0, 0, 1]
        put(e, model, [b""], [3])
        check(e, model, range(16))
    finally:
        e.close()


def test_a_bad_span_is_refused_with_its_index_and_stores_nothing(form):
    e, model = make(400, 1 << 16, form), Model(400, 1 << 16)
    try:
        put(e, model, [blob(10, 1)], [7])
        m = 300
        buf, off, ln = pack([blob(20, j) for j in range(m)])
        ids = np.arange(m, dtype=np.int32) + 10
        for at, (o, n) in ((290, (len(buf) - 19, 20)), (65, (-1, 3)), (131, (len(buf), 1))):
            off2, ln2 = off.copy(), ln.copy()
            off2[295], ln2[295] = len(buf), 5                  # a later bad record: the lowest index is named
            off2[at], ln2[at] = o, n
            st, res = e.cmds_put(packed=(buf, off2, ln2), triple_id=ids)
            assert st == EINVAL and list(res) == [-1, at, 0, 0]
            check(e, model, list(range(12)) + [at + 10, 11, 309])
        # a record that is not considered may say anything; a span that ends where the buffer ends is fine
        off2, ln2, ids2 = off.copy(), ln.copy(), ids.copy()
        off2[3], ids2[3] = 1 << 40, -1
        off2[4], ln2[4] = -5, -1
        off2[9], ln2[9] = len(buf), 0
        st, res = e.cmds_put(packed=(buf, off2, ln2), triple_id=ids2)
        assert st == 0 and list(res) == [m - 2, 20 * (m - 3), 0, 0]
        assert e.cmds_read(19) == b"" and e.cmds_read(13) is None and e.cmds_read(14) is None and e.cmds_read(15) == blob(20, 5)
    finally:
        e.close()


def test_both_copy_forms_give_the_same_arena():
    rng = np.random.default_rng(7)
    m = 700
    commands = [blob(int(n), j) for j, n in enumerate(rng.integers(0, 400, size=m))] + [blob(MAX_LEN, 3), blob(4097, 4)]
    ids = list(rng.integers(0, 500, size=len(commands)).astype(int))
    got = []
    for bytewise in (False, True):
        e, model = make(512, 1 << 20, bytewise), Model(512, 1 << 20)
        try:
            put(e, model, commands, ids, lead=5, gap=3)
            got.append(([e.cmds_read(t) for t in range(512)], e.cmds_stats()))
            assert arena_of(e, model) == model.arena
        finally:
            e.close()
    assert got[0] == got[1]


def test_put_dev_stands_back_behind_a_raised_status_and_m_zero():
    import torch

    from frankenpaxos_amd._lib import FpxError

    e = make(8, 256)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off, ln = pack([b"abc", b"defgh"])
        up = lambda a: torch.from_numpy(a.copy()).to(dev)
        d = [up(buf), up(off), up(ln), up(np.array([1, 2], np.int32))]
        res = torch.full((4,), -9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # a bad span raises FPX_EINVAL on the context; the put enqueued behind it stands back
        bad = up(np.array([0, 99], np.int64))
        e.cmds_put_dev(d[0], bad, d[2], d[3], res)
        res2 = torch.full((4,), -9, dtype=torch.int64, device=dev)
        e.cmds_put_dev(*d, res2)
        assert e.sync() == EINVAL and res.cpu().tolist() == [-1, 1, 0, 0] and res2.cpu().tolist() == [0, 0, 0, 0]
        assert e.cmds_stats() == (0, 0, 0, 0)
        e.cmds_put_dev(*d, res2)
        assert e.sync() == 0 and res2.cpu().tolist() == [2, 8, 0, 0]
        assert e.cmds_read(1) == b"abc" and e.cmds_read(2) == b"defgh" and e.cmds_read(0) is None
        st, r = e.cmds_put([], [])
        assert st == 0 and list(r) == [0, 0, 0, 0]
        with pytest.raises(FpxError):
            e.cmds_enable(8, 256)                              # a second call
        with pytest.raises(FpxError):
            e.cmds_read(8)
    finally:
        e.close()
    from frankenpaxos_amd.epaxos import EPaxos

    plain = EPaxos(3, 4, num_instances=8)
    try:
        with pytest.raises(FpxError):
            plain.cmds_stats()
        assert plain.cmds_put([b"a"], [0])[0] == EINVAL
    finally:
        plain.close()
