"""K4: Mencius noop ranges:
mencius/Acceptor.scala:237-291, mencius/ProxyLeader.scala:255-303, 355-411."""
import numpy as np
import pytest

from tests import workloads as W

pytestmark = pytest.mark.usefixtures("row_layout")

L, A, R = 3, 2, 3  # leader groups, acceptor groups per leader group, acceptors per group (f = 1)
KW = dict(num_slots=256, num_replicas=R, num_groups=A, num_leader_groups=L, f=1, tally_ways=8)


def test_oracle_noop_range_by_hand(oracle):
    s = oracle.System(oracle.make_config(**KW))
    # leader group 1 owns slots 1, 4, 7, 10, ...; acceptor group of slot = (slot / 3) % 2:
    # 1 -> 0, 4 -> 1, 7 -> 0, 10 -> 1, 13 -> 0
    # acceptor (lg 1, ag 0, idx 2) was promised round 5 by someone else
    assert s.acceptor_phase1a(1 * A + 0, 5, 0, oracle.bits_of([2]))[0] == 0
    st, vb, nb, nr = s.acceptor_phase2a_noop_range(4, 14, 2)
    assert st == 0 and nr == 5
    assert oracle.indices_of(vb[0]) == [0, 1] and oracle.indices_of(nb[0]) == [2]   # ag 0
    assert oracle.indices_of(vb[1]) == [0, 1, 2] and oracle.indices_of(nb[1]) == []  # ag 1
    vr, vv, _ = s.read_state()
    assert vr[7].tolist() == [2, 2, -1] and vr[13].tolist() == [2, 2, -1]       # ag 0 slots in [4, 14)
    assert vr[4].tolist() == [2, 2, 2] and vr[10].tolist() == [2, 2, 2]        # ag 1 slots
    assert (vv[[4, 7, 10, 13]][vr[[4, 7, 10, 13]] == 2] == -1).all()            # Noop
    assert (vr[[1, 5, 6, 8, 16]] == -1).all()                                   # outside / other leader groups
    pr, mv = s.read_scalars()
    assert pr[2].tolist() == [2, 2, 5] and pr[3].tolist() == [2, 2, 2] and (pr[[0, 1, 4, 5]] == -1).all()
    assert mv[2].tolist() == [13, 13, -1] and mv[3].tolist() == [10, 10, 10]
    # proxy leader: a quorum (f + 1 = 2) from EVERY acceptor group
    assert s.proxy_phase2b_noop_range(4, 14, 2, vb)[0] == 2                      # never opened: fatal
    assert s.proxy_open_noop_range(4, 14, 2) == (0, 1)
    assert s.proxy_open_noop_range(4, 14, 2) == (0, 0)                           # known: ignored
    one = np.zeros((A, 4), np.uint64)
    one[0] = oracle.bits_of([0, 1])
    assert s.proxy_phase2b_noop_range(4, 14, 2, one) == (0, 0)                   # ag 1 has no votes yet
    one[0] = 0
    one[1] = oracle.bits_of([2])
    assert s.proxy_phase2b_noop_range(4, 14, 2, one) == (0, 0)                   # ag 1: 1 < 2
    one[1] = oracle.bits_of([2, 0])
    assert s.proxy_phase2b_noop_range(4, 14, 2, one) == (0, 1)                   # ChosenNoopRange
    assert s.proxy_phase2b_noop_range(4, 14, 2, one) == (0, 0)                   # Done: ignored


def test_oracle_length_one_range_collides_with_single_slot_key(oracle):
    """SlotRound(slot, slot + 1, round) is the key of both (mencius/ProxyLeader.scala:86-90)"""
    s = oracle.System(oracle.make_config(**KW))
    i32 = lambda x: np.array([x], np.int32)
    assert s.proxy_open(i32(7), i32(0), i32(55))[1][0] == 1
    assert s.proxy_open_noop_range(7, 8, 0) == (0, 0)          # single-slot Phase2a pending: ignored
    votes = np.zeros((A, 4), np.uint64)
    votes[:] = oracle.bits_of([0, 1, 2])
    assert s.proxy_phase2b_noop_range(7, 8, 0, votes) == (0, 0)  # swallowed by the PendingPhase2a
    assert s.proxy_open_noop_range(10, 11, 3) == (0, 1)
    assert s.proxy_open(i32(10), i32(3), i32(1))[1][0] == 0    # the range owns the key
    st, ch, cr, cv = s.proxy_phase2b(i32(10), i32(3), W.bits_from_bool(np.ones((1, 3), bool)))
    assert st == 0 and ch[0] == 0                              # PendingPhase2aNoopRange: ignored
    assert s.proxy_phase2b_noop_range(10, 11, 3, votes) == (0, 1)


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.mark.gpu
def test_noop_ranges_match_oracle(fa, oracle):
    gpu = fa.Context(fa.make_config(**KW))
    ref = oracle.System(oracle.make_config(**KW))
    rng = np.random.default_rng(5)
    S = KW["num_slots"]
    i32 = lambda x: np.array(x, np.int32)
    for step in range(120):
        kind = rng.integers(0, 6)
        lg = int(rng.integers(0, L))
        start = lg + L * int(rng.integers(0, S // L - 2))
        end = min(S, start + L * int(rng.integers(0, 12)) + int(rng.integers(0, 2)) * (1 - L))
        end = max(end, start)
        rnd = int(rng.integers(0, 4))
        if kind == 0:    # a competing leader's Phase1a on some acceptors
            g = int(rng.integers(0, L * A))
            t = W.bits_from_bool(W.random_subsets(rng, 1, R, 1, R))[0]
            assert gpu.acceptor_phase1a(g, rnd, 0, t)[0] == ref.acceptor_phase1a(g, rnd, 0, t)[0]
        elif kind in (1, 2):
            tm = W.bits_from_bool(W.random_subsets(rng, A, R, 1, R)) if kind == 2 else None
            a = gpu.acceptor_phase2a_noop_range(start, end, rnd, tm)
            b = ref.acceptor_phase2a_noop_range(start, end, rnd, tm)
            assert a[0] == b[0] and a[3] == b[3]
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2], b[2])
            assert gpu.proxy_open_noop_range(start, end, rnd) == ref.proxy_open_noop_range(start, end, rnd)
            half = a[1].copy()
            half[:, 0] &= np.uint64(rng.integers(0, 8))
            for votes in (half, a[1], a[1]):
                assert gpu.proxy_phase2b_noop_range(start, end, rnd, votes) == \
                    ref.proxy_phase2b_noop_range(start, end, rnd, votes)
        elif kind == 3:  # ordinary single-slot traffic interleaved, including colliding keys
            slots = i32(sorted(set(rng.integers(0, S, 20).tolist()) | {start}))
            rr = np.full(len(slots), rnd, np.int32)
            W.assert_same_outputs(W.run_script(gpu, [("fused", slots, rr, slots * 3, None)]),
                                  W.run_script(ref, [("fused", slots, rr, slots * 3, None)]))
        elif kind == 4:  # length-one ranges
            assert gpu.proxy_open_noop_range(start, start + 1, rnd) == ref.proxy_open_noop_range(start, start + 1, rnd)
            votes = np.zeros((A, 4), np.uint64)
            votes[:] = oracle.bits_of([0, 1, 2])
            assert gpu.proxy_phase2b_noop_range(start, start + 1, rnd, votes) == \
                ref.proxy_phase2b_noop_range(start, start + 1, rnd, votes)
            vb = W.bits_from_bool(np.ones((1, 3), bool))
            a = gpu.proxy_phase2b(i32([start]), i32([rnd]), vb)
            b = ref.proxy_phase2b(i32([start]), i32([rnd]), vb)
            assert a[0] == b[0] and a[1][0] == b[1][0]
        else:            # Phase2bNoopRange for a key nobody opened: fatal
            votes = np.zeros((A, 4), np.uint64)
            votes[0] = oracle.bits_of([1])
            a = gpu.proxy_phase2b_noop_range(start, end + 1000 if end + 1000 <= S else end, 9, votes)
            b = ref.proxy_phase2b_noop_range(start, end + 1000 if end + 1000 <= S else end, 9, votes)
            assert a == b
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, 7))


@pytest.mark.gpu
def test_noop_range_arguments(fa):
    gpu = fa.Context(fa.make_config(**KW))
    assert gpu.acceptor_phase2a_noop_range(5, 4, 0)[0] == fa.FPX_EINVAL
    assert gpu.acceptor_phase2a_noop_range(0, 257, 0)[0] == fa.FPX_EINVAL
    assert gpu.proxy_open_noop_range(0, 4, -1)[0] == fa.FPX_EINVAL
    per_slot = fa.Context(fa.make_config(ballot_mode=1, **KW))
    assert per_slot.acceptor_phase2a_noop_range(0, 4, 0)[0] == fa.FPX_EINVAL


# ------------------------------------------------ the receiver: Replica.handleChosenNoopRange ------
def test_oracle_replica_chosen_noop_range_by_hand(oracle):
    """mencius/Replica.scala:464-485, including its early `return` on a slot that is already chosen"""
    s = oracle.System(oracle.make_config(**KW))            # 3 leader groups: stride 3
    assert s.replica_chosen_noop_range(1, 11) == (0, 0, 4)  # slots 1, 4, 7, 10 <- Noop; hole at 0
    vals, pres = s.replica_read_log(0, 12)
    assert pres.tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0] and (vals[pres == 1] == -1).all()
    assert s.replica_chosen([0, 2, 3], [50, 52, 53])[1:] == (5, 7)   # prefix 0..4 executes
    # leader group 2 skips 2, 5, 8, 11 -- but 2 is already chosen: the handler returns at once,
    # nothing is put and executeLog does not run
    assert s.replica_chosen_noop_range(2, 12) == (0, 5, 7)
    assert s.replica_read_log(5, 1)[1].tolist() == [0]
    # from 5 on: 5, 8, 11 are put; executeLog: 5 -> watermark 6 (6 is missing)
    assert s.replica_chosen_noop_range(5, 12) == (0, 6, 10)
    # a range that hits a chosen slot in the middle: 13 is put, 16 is present -> return; 19 is NOT put,
    # and executeLog is skipped although nothing blocks it
    assert s.replica_chosen([16, 6], [66, 56])[1:] == (9, 12)
    assert s.replica_chosen([9], [59])[1:] == (12, 13)
    assert s.replica_chosen([12], [62])[1:] == (13, 14)
    assert s.replica_chosen_noop_range(13, 22) == (0, 13, 15)       # 13 put, watermark NOT advanced
    assert s.replica_read_log(19, 1)[1].tolist() == [0]
    assert s.replica_chosen_noop_range(30, 30) == (0, 14, 15)       # empty range: executeLog only
    assert s.replica_chosen_noop_range(-1, 4)[0] == 1 and s.replica_chosen_noop_range(0, 257)[0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 3])
def test_replica_chosen_noop_range_matches_oracle(fa, oracle, stride):
    kw = dict(KW, num_leader_groups=stride, num_slots=4096)
    gpu = fa.Context(fa.make_config(**kw))
    ref = oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(17 + stride)
    S = kw["num_slots"]
    for step in range(300):
        if rng.random() < 0.5:
            n = int(rng.integers(1, 40))
            slot = rng.integers(0, min(S, 64 + step * 14), n).astype(np.int32)
            val = rng.integers(0, 1000, n).astype(np.int32)
            assert gpu.replica_chosen(slot, val) == ref.replica_chosen(slot, val)
        else:
            start = int(rng.integers(0, min(S - 1, 32 + step * 14)))
            end = min(S, start + int(rng.integers(0, 200)))
            assert gpu.replica_chosen_noop_range(start, end) == ref.replica_chosen_noop_range(start, end)
    a, b = gpu.replica_read_log(0, S), ref.replica_read_log(0, S)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0][a[1] == 1], b[0][b[1] == 1])
    assert gpu.replica_chosen_noop_range(0, S + 1)[0] == fa.FPX_EINVAL


# ------------------------------------------------ batches of ranges (K4 at Mencius scale) ------------------
def _random_range_batch(rng, S, L, n, rounds, dup=0.15):
    """n ranges of random leader groups; one round per leader group within the batch (rounds[lg]); some exact
    duplicates, some overlaps"""
    lg = rng.integers(0, L, n)
    rows = S // L
    first = rng.integers(0, rows - 1, n)
    length = rng.integers(0, 40, n)
    start = (first * L + lg).astype(np.int32)
    end = np.minimum(S, start + length * L + rng.integers(0, 2, n) * (1 - L)).astype(np.int32)
    end = np.maximum(end, start).astype(np.int32)
    for i in range(1, n):
        if rng.random() < dup:
            j = int(rng.integers(0, i))
            start[i], end[i], lg[i] = start[j], end[j], lg[j]
    rnd = np.array([rounds[int(x)] for x in lg], np.int32)
    return start, end, rnd


def test_oracle_batched_ranges_are_the_singles_in_order(oracle):
    """the oracle's batched / fused forms are nothing but the single-message handlers applied in array order"""
    kw = dict(num_slots=3000, num_replicas=3, num_groups=2, num_leader_groups=5, f=1, tally_ways=8)
    a, b = oracle.System(oracle.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(8)
    rounds = [0] * 5
    for step in range(30):
        if step % 7 == 6:
            lg = int(rng.integers(0, 5))
            rounds[lg] += int(rng.integers(1, 3))
        start, end, rnd = _random_range_batch(rng, 3000, 5, 25, rounds)
        tm = W.bits_from_bool(W.random_subsets(rng, 25 * 2, 3, 1, 3)).reshape(25, 2, 4)
        st, vb, nb, nr, new, ch = a.noop_ranges_fused(start, end, rnd, tm)
        assert st == 0
        for i in range(25):
            s, e, r = int(start[i]), int(end[i]), int(rnd[i])
            st1, fresh = b.proxy_open_noop_range(s, e, r)
            assert fresh == new[i]
            if fresh:
                st2, vb1, nb1, nr1 = b.acceptor_phase2a_noop_range(s, e, r, tm[i])
                np.testing.assert_array_equal(vb1, vb[i])
                np.testing.assert_array_equal(nb1, nb[i])
                assert nr1 == nr[i]
                assert b.proxy_phase2b_noop_range(s, e, r, vb1) == (0, ch[i])
            else:
                assert ch[i] == 0 and not vb[i].any()
        np.testing.assert_array_equal(a.state_digest(), b.state_digest())


def test_oracle_ranges_with_more_than_256_acceptors_per_leader_group(oracle):
    """num_groups x R > 256: the votes of a range are one 256-bit set per acceptor group"""
    kw = dict(num_slots=4000, num_replicas=100, num_groups=4, num_leader_groups=2, f=49)
    s = oracle.System(oracle.make_config(**kw))
    st, vb, nb, nr, new, ch = s.noop_ranges_fused([1], [801], [3])
    assert st == 0 and new[0] == 1 and ch[0] == 1 and (vb[0, :, 0] == np.uint64(2 ** 64 - 1)).all()
    assert [bin(int(x)).count("1") for x in vb[0, :, 1]] == [36] * 4
    assert s.read_range_tally(1, 801, 3)[0] == 2
    tm = np.zeros((1, 4, 4), np.uint64)
    tm[0, :, 0] = np.uint64((1 << 50) - 1)           # 50 = f + 1 acceptors of each group ...
    tm[0, 2, 0] = np.uint64((1 << 49) - 1)           # ... but only 49 of group 2
    st, vb, nb, nr, new, ch = s.noop_ranges_fused([1001], [1201], [3], tm)
    assert new[0] == 1 and ch[0] == 0
    state, votes = s.read_range_tally(1001, 1201, 3)
    assert state == 1 and [bin(int(x)).count("1") for x in votes[:, 0]] == [50, 50, 49, 50]
    late = np.zeros((1, 4, 4), np.uint64)
    late[0, 2, 0] = np.uint64(1 << 60)
    st, ch = s.proxy_phase2b_noop_ranges([1001], [1201], [3], late)
    assert st == 0 and ch.tolist() == [1]
    vr, vv, _ = s.read_state()
    assert vr[1005, :49].tolist() == [3] * 49 and vr[1005, 49] == -1    # slot 1005: acceptor group (1005 / 2) % 4 = 2
    assert vr[1001, :50].tolist() == [3] * 50 and vr[1001, 50] == -1    # slot 1001: acceptor group 0


def _same_ranges(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.gpu
@pytest.mark.parametrize("L,A,R,f", [(5, 2, 3, 1), (256, 1, 3, 1), (2, 4, 100, 49), (7, 3, 5, 2)])
def test_batched_ranges_match_oracle(fa, oracle, L, A, R, f):
    """fused batches of ranges (duplicates inside a batch, overlaps, leader groups in different rounds, partial
    target masks, Nacks from competing leaders), the unfused batched entry points, single-slot traffic in between,
    garbage collection -- every output, the whole acceptor state, and every range tally"""
    S = 1 << 15
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=f, tally_ways=8)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(L * 100 + A * 10 + R)
    rounds = [0] * L
    seen = []
    for step in range(24):
        n = int(rng.integers(1, 200))
        if step % 5 == 4:        # a competing leader of some groups: Phase1a in a higher round on a few acceptors
            for _ in range(3):
                lg = int(rng.integers(0, L))
                g = lg * A + int(rng.integers(0, A))
                t = W.bits_from_bool(W.random_subsets(rng, 1, R, 1, max(1, R // 2)))[0]
                _same_ranges(gpu.acceptor_phase1a(g, rounds[lg] + 1, 0, t), ref.acceptor_phase1a(g, rounds[lg] + 1, 0, t))
        if step % 6 == 5:        # leader changes: some leader groups move on to higher rounds
            for lg in rng.integers(0, L, 3):
                rounds[int(lg)] += 2
        start, end, rnd = _random_range_batch(rng, S, L, n, rounds)
        kind = step % 4
        if kind in (0, 1):
            tm = None if kind == 0 else W.bits_from_bool(W.random_subsets(rng, n * A, R, f + 1, R)).reshape(n, A, 4)
            _same_ranges(gpu.noop_ranges_fused(start, end, rnd, tm), ref.noop_ranges_fused(start, end, rnd, tm))
        elif kind == 2:
            a, b = gpu.proxy_open_noop_ranges(start, end, rnd), ref.proxy_open_noop_ranges(start, end, rnd)
            _same_ranges(a, b)
            a, b = gpu.acceptor_phase2a_noop_ranges(start, end, rnd), ref.acceptor_phase2a_noop_ranges(start, end, rnd)
            _same_ranges(a, b)
            half = a[1].copy()
            half[:, :, 0] &= np.uint64(rng.integers(0, 8))
            for votes in (half, a[1], a[1]):
                _same_ranges(gpu.proxy_phase2b_noop_ranges(start, end, rnd, votes),
                             ref.proxy_phase2b_noop_ranges(start, end, rnd, votes))
        else:                    # single-slot commands of the same leader groups, colliding with length-1 ranges
            slots = np.unique(np.concatenate([start, rng.integers(0, S, 50).astype(np.int32)])).astype(np.int32)
            rr = np.array([rounds[int(s) % L] for s in slots], np.int32)
            W.assert_same_outputs(W.run_script(gpu, [("fused", slots, rr, slots * 3, None)]),
                                  W.run_script(ref, [("fused", slots, rr, slots * 3, None)]))
            ones = np.ones(n, np.int32)
            _same_ranges(gpu.noop_ranges_fused(start, start + ones, rnd), ref.noop_ranges_fused(start, start + ones, rnd))
        seen.append((start, end, rnd))
        if step == 15:           # garbage-collect the lower half of the window, tallies of ranges inside it included
            gpu.proxy_forget(0, S // 2)
            ref.proxy_forget(0, S // 2)
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, 509))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    for start, end, rnd in seen[::3]:
        for i in range(0, len(start), 7):
            a = gpu.read_range_tally(int(start[i]), int(end[i]), int(rnd[i]))
            b = ref.read_range_tally(int(start[i]), int(end[i]), int(rnd[i]))
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])


@pytest.mark.gpu
def test_range_tallies_are_reclaimed(fa, oracle):
    """ADVICE r01 / VERDICT r01 weak #8: a long-running proxy leader opens far more than 1024 ranges; Done and
    Pending entries of a garbage-collected window are freed, so the table never fills up"""
    L, S = 16, 1 << 16
    kw = dict(num_slots=S, num_replicas=3, num_groups=1, num_leader_groups=L, f=1)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    win = 4096
    total = 0
    for lap in range(3):
        for w in range(S // win):
            start = (np.arange(win // 2, dtype=np.int32) * 2 + w * win)            # 2048 ranges of 2 slots' width
            end = np.minimum(start + 2 * L, (w + 1) * win).astype(np.int32)
            rnd = np.full(len(start), lap, np.int32)
            _same_ranges(gpu.noop_ranges_fused(start, end, rnd), ref.noop_ranges_fused(start, end, rnd))
            total += len(start)
            gpu.proxy_forget(w * win, win)
            ref.proxy_forget(w * win, win)
    assert total > 90000
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    # without garbage collection the table does fill: loud, not silent
    st = 0
    for k in range(40):
        start = (np.arange(2048, dtype=np.int32) * 16 + k % 16)
        st = gpu.noop_ranges_fused(start, start + 16 * (k // 16 + 1), np.full(2048, 3, np.int32))[0]
        if st:
            break
    assert st == fa.FPX_ECAPACITY


@pytest.mark.gpu
def test_slot_major_flag_gives_the_same_state(fa, oracle, row_layout, monkeypatch):
    """FPX_F_SLOT_MAJOR_ROWS (include/fpx.h) changes where a slot's row lives, nothing else: commands, noop ranges,
    garbage collection and recycling on two contexts that differ only in the flag, and on the oracle.  The context
    without the flag is created without the FPX_SLOT_MAJOR switch, so that its rows stay leader-group-major; under the
    slot-major layout a third context, without the flag, takes its slot-major rows from the switch."""
    S, L = 1 << 14, 8
    kw = dict(num_slots=S, num_replicas=3, num_groups=2, num_leader_groups=L, f=1, tally_ways=8)
    with monkeypatch.context() as m:
        m.delenv("FPX_SLOT_MAJOR", raising=False)
        a = fa.Context(fa.make_config(**kw))
    ctxs = [a, fa.Context(fa.make_config(flags=fa.FPX_F_SLOT_MAJOR_ROWS, **kw))]
    if row_layout == "slot-major":
        ctxs.append(fa.Context(fa.make_config(**kw)))
    ref = oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(77)
    for step in range(6):
        slots = np.unique(rng.integers(0, S, 3000)).astype(np.int32)
        rr = np.full(len(slots), step // 3, np.int32)
        tm = W.bits_from_bool(W.random_subsets(rng, len(slots), 3, 1, 3))
        script = [("fused", slots, rr, slots * 7 + step, tm)]
        want = W.run_script(ref, script)
        for x in ctxs:
            W.assert_same_outputs(W.run_script(x, script), want)
        start, end, rnd = _random_range_batch(rng, S, L, 60, [step // 3] * L)
        want = ref.noop_ranges_fused(start, end, rnd)
        for x in ctxs:
            _same_ranges(x.noop_ranges_fused(start, end, rnd), want)
        if step == 3:
            for x in ctxs + [ref]:
                x.proxy_forget(100, S // 3)
                x.recycle_slots(S // 2 + 3, 1000)
    for x in ctxs:
        W.assert_same_state(x, ref, tally_slots=range(0, S, 37))
        np.testing.assert_array_equal(x.state_digest(), ref.state_digest())


@pytest.mark.gpu
@pytest.mark.parametrize("L,A,R", [(8, 1, 3), (12, 2, 4), (6, 1, 3), (256, 1, 3), (16, 1, 8)])
def test_slot_ordered_batches_are_walked_by_column(fa, oracle, L, A, R):
    """a batch in slot order across the leader groups (message i + P is the next slot of message i's leader group): on
    leader-group-major rows k_phase2 walks it column by column -- four columns at a time when P is a multiple of 4 --
    with a tail of plain chunks; dense and with target masks, fused and unfused, some leader groups silent (P < L),
    leader groups in different rounds; every output and the whole state against the oracle"""
    S = L * max(1024, -(-65536 // L))
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=(R - 1) // 2, tally_ways=8)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(L * 7 + R)
    rounds = rng.integers(0, 3, L)
    lo = 0
    for step in range(6):
        n = int(rng.integers(3000, 9000))
        slots = np.arange(lo, min(S, lo + n), dtype=np.int32)
        lo += n // 2                                  # the next batch re-proposes half of this one (known (slot, round))
        if step % 3 == 2:                             # every other leader group is silent: the period halves
            slots = slots[(slots % L) % 2 == 0]
        if step == 4:
            rounds = rounds + 1
        rr = rounds[slots % L].astype(np.int32)
        val = (slots * 11 + step).astype(np.int32)
        tm = None if step % 2 == 0 else W.bits_from_bool(W.random_subsets(rng, len(slots), R, 1, R))
        if step == 3:
            script = [("k1k2", slots, rr, val, tm, rng.random(len(slots)) < 0.1)]
        else:
            script = [("fused", slots, rr, val, tm)]
        W.assert_same_outputs(W.run_script(gpu, script), W.run_script(ref, script))
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, max(1, S // 200)))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2048, 1500])
def test_row_sweep_fill_with_two_thousand_leader_groups(fa, oracle, row_layout, L):
    """on slot-ordered rows (FPX_F_SLOT_MAJOR_ROWS) the noop-range fill that sweeps 8 log rows with an LDS
    ownership map (k_ranges_fill_rows) needs 8 x L x 4 B of dynamic LDS + its static words: beyond the default 64 KiB at
    L close to 2048 -- without the opt-in every fused range call failed with FPX_EHIP instead of working.  The rows are
    slot-ordered by the flag, or under the slot-major layout by the FPX_SLOT_MAJOR switch alone."""
    S = L * 16
    kw = dict(num_slots=S, num_replicas=3, num_groups=1, num_leader_groups=L, f=1, tally_ways=4)
    flags = 0 if row_layout == "slot-major" else fa.FPX_F_SLOT_MAJOR_ROWS
    gpu, ref = fa.Context(fa.make_config(flags=flags, **kw)), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(L)
    for step in range(3):
        start, end, rnd = _random_range_batch(rng, S, L, 300, [step] * L)
        _same_ranges(gpu.noop_ranges_fused(start, end, rnd), ref.noop_ranges_fused(start, end, rnd))
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, 511))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
