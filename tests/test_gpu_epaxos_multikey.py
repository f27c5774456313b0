"""Multi-key get / set commands on the device (the _mk entry points of include/fpx.h) against
tests/epaxos_multikey_sets.py (explicit sets), a vectorized numpy restatement at size, and the single-key forms."""
import numpy as np
import pytest

from tests import epaxos_multikey_sets as mk
from tests.test_epaxos_models import decode
from tests.test_epaxos_multikey_model import load_golden
from tests.workloads import random_tick

pytestmark = pytest.mark.gpu


def random_keys(rng, m, num_keys, lo=0, hi=6):
    """0..6 keys per command, repeats included"""
    return [list(rng.integers(0, num_keys, int(c))) for c in rng.integers(lo, hi + 1, m)]


def seen_of(rng, n, leader, mask):
    others = np.array([((1 << n) - 1) & ~(1 << int(L)) for L in leader], np.uint8)
    extra = np.array([rng.random() < 0.5 for _ in leader])
    return np.where(extra, others, mask).astype(np.uint8)


def test_device_reproduces_the_reference_k1_vectors():
    from frankenpaxos_amd.epaxos import EPaxos

    g, puts, queries = load_golden()
    n = g["num_leaders"]
    for qi, (keys, is_set, top) in enumerate(queries):
        e = EPaxos(n, len(g["keys"]), num_instances=32)
        order = np.random.default_rng(qi).permutation(len(puts))        # puts are maxima: any order
        P = [puts[j] for j in order]
        st = e.handle_commit_mk([p[0][0] for p in P], [p[0][1] for p in P], list(range(len(P))), [1] * len(P),
                                [list(p[1]) for p in P], [int(p[2]) for p in P])
        assert st == 0
        # a fresh instance numbered above every top: subtractOne removes nothing, the deps ARE the TopOne vector
        r = e.handle_preaccept_mk([0], [25], [0], [0], [list(keys)], [int(is_set)], [99], np.zeros((1, n)), None, [1])
        assert r[0] == 0 and r[1][0] == 1
        assert r[6][0][0].tolist() == top, (keys, is_set)
        e.close()


def check_tick(e, ref, n, rng, m, num_keys, form, seen, NI, fifo, nxt):
    import torch

    leader, number, _, is_set, mask, rank = random_tick(rng, n, num_keys, m, nxt, 5.0, fifo=fifo)
    keys = random_keys(rng, m, num_keys)
    sm = seen_of(rng, n, leader, mask) if seen else None
    tid = np.arange(m, dtype=np.int32) + 1000 * int(number.max()) if NI else None
    want = ref.tick(leader, number, [tuple(k) for k in keys], is_set, mask, rank, seen_mask=sm, triple_id=tid)
    off, ks = mk.csr(keys)
    if form == "host":
        st, fast, deps, ldeps, own = e.preaccept_mk(leader, number, keys, is_set, mask, rank, seen_mask=sm, triple_id=tid)
        assert st == 0
    else:
        T = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
        args = [T(leader), T(number), T(off), T(ks if len(ks) else np.zeros(1, np.int32)), T(is_set, torch.uint8),
                T(mask, torch.uint8), T(rank)]
        kw = dict(seen_mask=None if sm is None else T(sm, torch.uint8), triple_id=None if tid is None else T(tid))
        if form == "dev":
            fast_t, deps_t = torch.zeros(m, dtype=torch.uint8, device="cuda"), torch.zeros((m, n), dtype=torch.int32, device="cuda")
            ldeps_t, own_t = torch.zeros((m, n), dtype=torch.int32, device="cuda"), torch.zeros((m, 2), dtype=torch.int32, device="cuda")
            e.preaccept_mk_dev(*args, fast=fast_t, deps=deps_t, leader_deps=ldeps_t, own_values_end=own_t, **kw)
            assert e.sync() == 0
            fast, deps, ldeps, own = (t.cpu().numpy() for t in (fast_t, deps_t, ldeps_t, own_t))
        else:
            packed = torch.zeros((m, e.packed_stride()), dtype=torch.int32, device="cuda")
            e.preaccept_mk_packed_dev(*args, packed, **kw)
            assert e.sync() == 0
            fast, deps, ldeps, own = (np.asarray(a) for a in e.unpack(packed.cpu().numpy()))
    for i in range(m):
        L, x = int(leader[i]), int(number[i])
        wf, wd, wD = want[i]
        assert bool(fast[i]) == wf, i
        assert decode(deps[i], L, x, own[i][0]) == wd, i
        assert decode(ldeps[i], L, x, own[i][1]) == wD, i
        if NI:
            for r in range(n):
                ent = ref.replicas[r].cmd_log.get((L, x))
                kind, _, _, t, _ = e.read_cmdlog(r, L, x)
                assert kind == (0 if ent is None else ent.kind), (i, r)
                if ent is not None:
                    assert t == ent.triple_id
                    d, end = e.read_cmdlog_deps(r, L, x)
                    assert decode(d, L, x, end) == set(ent.deps), (i, r)
    return sum(len(set(k)) < len(k) for k in keys), sum(len(k) == 0 for k in keys)


@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("NI", [0, 1])
@pytest.mark.parametrize("seen", [False, True])
def test_multikey_ticks_match_the_set_model(n, NI, seen):
    from frankenpaxos_amd.epaxos import EPaxos

    num_keys, m = 12, 224
    reps = zeros = 0
    for seed, form in enumerate(("host", "dev", "packed")):
        rng = np.random.default_rng(100 * n + 10 * NI + 2 * seed + seen)
        e = EPaxos(n, num_keys, num_instances=(4 * m if NI else 0))
        ref = mk.EPaxos(n, num_keys)
        nxt = [0] * n
        for tick in range(2):
            a, b = check_tick(e, ref, n, rng, m, num_keys, form, seen, NI, tick == 1, nxt)
            reps, zeros = reps + a, zeros + b
        for r in range(n):
            for k in range(num_keys):
                g, s = e.read_index(r, k)
                assert g.tolist() == ref.replicas[r].gets[k] and s.tolist() == ref.replicas[r].sets[k], (r, k)
        e.close()
    assert reps > 0 and zeros > 0


def _packed_dev(e, leader, number, key_or_off, keys, is_set, mask, rank, mk_form):
    import torch

    T = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    packed = torch.zeros((len(leader), e.packed_stride()), dtype=torch.int32, device="cuda")
    if mk_form:
        e.preaccept_mk_packed_dev(T(leader), T(number), T(key_or_off), T(keys), T(is_set, torch.uint8), T(mask, torch.uint8),
                                  T(rank), packed)
    else:
        e.preaccept_packed_dev(T(leader), T(number), T(key_or_off), T(is_set, torch.uint8), T(mask, torch.uint8), T(rank), packed)
    assert e.sync() == 0
    return packed.cpu().numpy()


def test_one_key_per_command_is_the_single_key_tick_bit_for_bit():
    from frankenpaxos_amd.epaxos import EPaxos

    n, num_keys, m = 5, 1024, 1 << 20
    a, b = EPaxos(n, num_keys), EPaxos(n, num_keys)
    rng = np.random.default_rng(7)
    nxt = [0] * n
    for tick, hot in enumerate((False, True)):   # the second tick has a hot key: the on-chip tables overflow
        leader, number, key, is_set, mask, rank = random_tick(rng, n, num_keys, m, nxt, 64.0, fifo=tick == 0)
        if hot:
            key[rng.random(m) < 0.05] = 3
        off = np.arange(m + 1, dtype=np.int32)
        pa = _packed_dev(a, leader, number, key, None, is_set, mask, rank, False)
        pb = _packed_dev(b, leader, number, off, key, is_set, mask, rank, True)
        np.testing.assert_array_equal(pa, pb)
    for r in range(n):
        for k in range(num_keys):
            ga, sa = a.read_index(r, k)
            gb, sb = b.read_index(r, k)
            assert ga.tolist() == gb.tolist() and sa.tolist() == sb.tolist()


def numpy_tick(n, num_keys, leader, number, off, keys, is_set, mask, rank, gets0, sets0):
    """vectorized restatement of a fresh thrifty tick (KeyValueStore.scala:221-302 per pair, max per command):
    -> (fast, deps, ldeps, own[m, 2], gets, sets) with gets / sets [num_keys][n] after the commit"""
    m = len(leader)
    cnt = np.diff(off)
    cmd = np.repeat(np.arange(m), cnt)
    # drop repeats inside a command: first occurrence of (cmd, key)
    _, first = np.unique(cmd.astype(np.int64) * num_keys + keys, return_index=True)
    uq = np.zeros(len(keys), bool)
    uq[first] = True
    pc, pk = cmd[uq], keys[uq].astype(np.int64)
    pL, pset, pid1 = leader[pc], is_set[pc].astype(bool), number[pc].astype(np.int64) + 1
    conf = np.zeros((m, n, n), np.int64)
    for r in range(n):
        part = (pL == r) | ((mask[pc].astype(np.int64) >> r) & 1).astype(bool)
        idx = np.nonzero(part)[0]
        o = np.lexsort((rank[r][pc[idx]], pk[idx]))
        idx = idx[o]
        seg = pk[idx]
        start = np.r_[True, seg[1:] != seg[:-1]]
        row = np.zeros((len(idx), n), np.int64)
        for l in range(n):
            for t, store in ((False, gets0), (True, sets0)):
                v = np.where((pL[idx] == l) & (pset[idx] == t), pid1[idx], 0)
                inc = np.maximum.accumulate(seg * 2**32 + v) - seg * 2**32
                exc = np.where(start, 0, np.r_[0, inc[:-1]])
                exc = np.maximum(exc, store[seg, l])
                if t:
                    row[:, l] = np.maximum(row[:, l], exc)
                else:
                    row[:, l] = np.where(pset[idx], np.maximum(row[:, l], exc), row[:, l])
        np.maximum.at(conf[:, r, :], pc[idx], row)
    ar = np.arange(m)
    D = conf[ar, leader]
    resp = [np.maximum(conf[:, r, :], D) for r in range(n)]
    fast = np.ones(m, bool)
    first = np.full((m, n), -1, np.int64)
    uni = D.copy()
    for r in range(n):
        inm = ((mask.astype(np.int64) >> r) & 1).astype(bool)
        uni = np.where(inm[:, None], np.maximum(uni, resp[r]), uni)
        fresh = inm & (first[:, 0] < 0)
        fast &= ~inm | fresh | (resp[r] == first).all(1)
        first = np.where(fresh[:, None], resp[r], first)
    w = np.where(fast[:, None], first, uni)
    x = number.astype(np.int64)

    def own(cols):
        c = cols[ar, leader]
        wm, end = np.where(c <= x, c, x), np.where(c > x + 1, c, 0)
        out = cols.copy()
        out[ar, leader] = wm
        return out, end

    deps, e0 = own(w)
    ldeps, e1 = own(D)
    gets, sets = gets0.copy(), sets0.copy()
    np.maximum.at(gets, (pk[~pset], pL[~pset]), pid1[~pset])
    np.maximum.at(sets, (pk[pset], pL[pset]), pid1[pset])
    return fast, deps, ldeps, np.stack([e0, e1], 1), gets, sets


def test_full_size_multikey_tick_matches_numpy():
    from frankenpaxos_amd.epaxos import EPaxos

    n, num_keys, m = 5, 1024, 1 << 20
    e = EPaxos(n, num_keys)
    rng = np.random.default_rng(11)
    nxt = [0] * n
    gets, sets = np.zeros((num_keys, n), np.int64), np.zeros((num_keys, n), np.int64)
    for tick in range(2):
        leader, number, _, is_set, mask, rank = random_tick(rng, n, num_keys, m, nxt, 64.0, fifo=tick == 0)
        cnt = rng.integers(1, 5, m)
        off = np.zeros(m + 1, np.int32)
        off[1:] = np.cumsum(cnt)
        keys = rng.integers(0, num_keys, int(off[-1])).astype(np.int32)
        p = _packed_dev(e, leader, number, off, keys, is_set, mask, rank, True)
        fast, deps, ldeps, own, gets, sets = numpy_tick(n, num_keys, leader, number, off, keys, is_set, mask, rank, gets, sets)
        np.testing.assert_array_equal(p[:, 2 * n + 2], fast.astype(np.int32))
        np.testing.assert_array_equal(p[:, :n], deps)
        np.testing.assert_array_equal(p[:, n:2 * n], ldeps)
        np.testing.assert_array_equal(p[:, 2 * n:2 * n + 2], own)
        assert 0 < int(fast.sum()) < m
    for r in range(n):
        for k in range(0, num_keys, 7):
            g, s = e.read_index(r, k)
            assert g.tolist() == gets[k].tolist() and s.tolist() == sets[k].tolist()


def test_multikey_slow_path_and_resent_preaccept_match_the_model():
    """PreAccept -> replicas answering differently -> Accept -> Commit, and a re-sent PreAccept, with key lists"""
    from frankenpaxos_amd.epaxos import EPaxos

    n, NK, NI = 5, 6, 16
    e, ref = EPaxos(n, NK, num_instances=NI), mk.EPaxos(n, NK)
    # history that differs between replicas: replica 1 saw set(0, 1) by (2, 0), replica 2 did not
    st = e.handle_preaccept_mk([2], [0], [0], [2], [[0, 1, 1]], [1], [7], np.zeros((1, n)), None, [0b010])
    ref.handle_preaccept((2, 0), (0, 2), (0, 1, 1), True, 7, set(), [1])
    assert st[0] == 0
    # a multi-key PreAccept of (0, 3) from leader 0 to replicas 1, 2, 3
    deps_in = np.zeros((1, n), np.int32)
    r = e.handle_preaccept_mk([0], [3], [0], [0], [[1, 4, 4]], [0], [11], deps_in, None, [0b1110])
    w = ref.handle_preaccept((0, 3), (0, 0), (1, 4, 4), False, 11, set(), [1, 2, 3])
    assert r[0] == 0 and r[1][0] == 0b1110
    answers = [decode(r[6][0][q], 0, 3, r[7][0][q]) for q in (1, 2, 3)]
    assert answers == [set(w[q][1]) for q in (1, 2, 3)]
    assert answers[0] != answers[1]                                   # the fast path is off: Accept
    # re-sent PreAccept in the same ballot: the stored reply comes back
    r2 = e.handle_preaccept_mk([0], [3], [0], [0], [[1, 4]], [0], [11], deps_in, None, [0b0010])
    w2 = ref.handle_preaccept((0, 3), (0, 0), (1, 4), False, 11, set(), [1])
    assert r2[2][0] == 0b0010 and w2[1][0] == "resend" and decode(r2[6][0][1], 0, 3, r2[7][0][1]) == set(w2[1][1])
    a = e.accept_mk([0], [3], [1], [0], [11], [0b0110], [[1, 4, 4]], [0])
    fatal, reps, committed = ref.accept((0, 3), (1, 0), 11, [1, 2], keys=(1, 4, 4), is_set=False)
    assert a[0] == 0 and not fatal and bool(a[5][0]) == committed
    e.handle_commit_mk([0], [3], [11], [0b11111], [[1, 4, 4]], [0])
    ref.handle_commit((0, 3), 11, None, range(n), keys=(1, 4, 4), is_set=False)
    # a zero-key command changes no index
    assert e.handle_commit_mk([4], [0], [12], [0b11111], [[]], [1]) == 0
    ref.handle_commit((4, 0), 12, None, range(n), keys=(), is_set=True)
    for rr in range(n):
        for k in range(NK):
            g, s = e.read_index(rr, k)
            assert g.tolist() == ref.replicas[rr].gets[k] and s.tolist() == ref.replicas[rr].sets[k], (rr, k)
        for (L, x), ent in ref.replicas[rr].cmd_log.items():
            kind, _, _, t, _ = e.read_cmdlog(rr, L, x)
            assert (kind, t) == (ent.kind, ent.triple_id), (rr, L, x)


def test_multikey_commits_execute_on_the_device():
    import torch
    from frankenpaxos_amd import depgraph as P
    from frankenpaxos_amd.epaxos import EPaxos
    from tests.test_depgraph_dev import check_valid_order, labels

    n, num_keys, m = 5, 64, 4096
    e = EPaxos(n, num_keys)
    rng = np.random.default_rng(5)
    nxt = [0] * n
    leader, number, _, is_set, mask, rank = random_tick(rng, n, num_keys, m, nxt, 8.0)
    off, keys = mk.csr(random_keys(rng, m, num_keys, 0, 4))
    packed = _packed_dev(e, leader, number, off, keys, is_set, mask, rank, True)
    first = [0] * n
    count = np.bincount(leader, minlength=n).tolist()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    order, comp = torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
    ne, nc, nh = e.execute_dev(T(leader), T(number), T(packed), first, count, order, comp)
    assert nh == 0 and ne == m
    order, comp = order.cpu().numpy(), comp.cpu().numpy()
    deps, own = packed[:, :n], packed[:, 2 * n:2 * n + 2]
    g = P.DependencyGraph(n, kind=P.FPX_DG_TARJAN)
    g.commit_epx(leader, number, deps, own)
    el, ei, cs, bl, bi = g.execute_arrays()
    assert len(el) == m and nc == len(cs)
    assert labels(n, leader, number, leader[order], number[order], comp) == \
        labels(n, leader, number, el, ei, np.repeat(np.arange(len(cs)), cs))
    check_valid_order(n, np.array(first), leader, number, deps, own[:, 0], order, comp)


def test_bad_key_lists_are_refused_and_nothing_is_applied():
    import torch
    from frankenpaxos_amd._lib import FpxError
    from frankenpaxos_amd.epaxos import EPaxos

    n, NK, NI = 3, 4, 8
    e = EPaxos(n, NK, num_instances=NI)
    leader, number, is_set = np.array([0, 1]), np.array([0, 0]), np.array([1, 0])
    mask = np.array([0b010, 0b100], np.uint8)
    rank = np.array([[0, 1], [0, 1], [1, 0]], np.int32)
    bad = [(np.array([0, 2, 1], np.int32), np.array([1, 2], np.int32)),              # not monotone
           (np.array([0, 1, 2], np.int32), np.array([1, NK], np.int32)),             # key out of range
           (np.array([0, 1, 2], np.int32), np.array([-1, 0], np.int32)),
           (np.array([1, 1, 2], np.int32), np.array([1, 2], np.int32))]              # key_offsets[0] != 0
    T = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    for off, keys in bad:
        assert e.preaccept_mk(leader, number, (off, keys), is_set, mask, rank)[0] == 1
        with pytest.raises(FpxError):
            e.preaccept_mk_dev(T(leader), T(number), T(off), T(keys), T(is_set, torch.uint8), T(mask, torch.uint8), T(rank))
        assert e.handle_preaccept_mk(leader, number, [0, 0], [0, 1], (off, keys), is_set, None, np.zeros((2, n)), None,
                                     [0b110, 0b101])[0] == 1
        assert e.accept_mk(leader, number, [1, 1], [0, 1], [5, 6], [0b010, 0b100], (off, keys), is_set)[0] == 1
        assert e.handle_commit_mk(leader, number, [5, 6], [0b111, 0b111], (off, keys), is_set) == 1
    # more pairs than FPX_EPX_MK_MAX_PAIRS
    big = np.array([0, 0, (1 << 23) + 1], np.int32)
    assert e.preaccept_mk(leader, number, (big, np.zeros((1 << 23) + 1, np.int32)), is_set, mask, rank)[0] == 1
    assert e.sync() == 0
    for r in range(n):
        for k in range(NK):
            g, s = e.read_index(r, k)
            assert not g.any() and not s.any()
        for L in range(n):
            assert e.read_cmdlog(r, L, 0)[0] == 0
    # and the same context still works
    assert e.preaccept_mk(leader, number, [[1, 1, 2], []], is_set, mask, rank)[0] == 0
