"""The leader half of EPaxos on the device (fpx_epx_lead, fpx_epx_leader_replies[_dev] with FPX_EPX_F_LEADER_STATE) against
tests/epaxos_leader_model.py, bit for bit on every output; the leader state, the command log and the conflict index are
compared through fpx_epx_read_leader_state / fpx_epx_read_cmdlog[_deps] / fpx_epx_read_index."""
import numpy as np
import pytest

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as S

pytestmark = pytest.mark.gpu


def ctx(n, num_keys=4, num_instances=64, leader_state=True):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, num_keys, num_instances=num_instances, leader_state=leader_state)


def both(n, ops, num_keys=4, num_instances=64):
    e, model = ctx(n, num_keys, num_instances), M.LeaderModel(n, num_keys, num_instances)
    got, want = S.run_gpu(e, ops), S.run_model(model, ops)
    assert got == want
    step = 1 + len(S.touched(ops)[0]) // 256                     # (a readback is a handful of small copies per cell)
    assert S.gpu_state(e, ops, step) == S.model_state(model, ops, step)
    e.close()
    return want


@pytest.mark.parametrize("n", [3, 5, 7])
def test_the_generators_streams(n):
    # every outcome code, both FPX_EFATAL_PROTOCOL sources, the four ways an instance is taken from its leader, a re-lead
    # after a Nack (tests/test_epaxos_leader_cpu.py asserts the histogram)
    both(n, S.make_stream(1, n))


def _ok(q, w, to=0, L=0, x=0, ballot=None, seq=0, end=0):
    ballot = (0, to) if ballot is None else ballot              # the default ballot of the replica that leads
    return (M.PRE_ACCEPT_OK, to, L, x, ballot[0], ballot[1], q, seq, list(w), end)


def test_quorum_sizes_at_3_5_and_7():
    for n, want in [(3, [M.FAST_COMMIT, M.IGNORED]),
                    (5, [M.WAITING, M.START_SLOW_PATH_TIMER, M.FAST_COMMIT, M.IGNORED]),
                    (7, [M.WAITING, M.WAITING, M.START_SLOW_PATH_TIMER, M.WAITING, M.FAST_COMMIT, M.IGNORED])]:
        ops = [("lead", [(0, 0, 0, 0, 1, 1, 7, 0)]), ("replies", [_ok(q, [0] * n) for q in range(1, n)])]
        res = both(n, ops)
        assert [r[0] for r in res[1][1]] == want and res[1][2] == [want.index(M.FAST_COMMIT)]


def test_several_hosted_leaders_and_one_number_under_different_leaders():
    n, z = 5, [0] * 5
    leads = [(L, 0, L, 0, 2, 1, 10 + L, 0) for L in range(n)] + [(1, 1, 3, 2, 2, 0, 20, 1)]
    burst = []
    for q in range(3):
        for L in range(n):
            burst.append(_ok((L + 1 + q) % n, z if (L, q) != (2, 1) else [0, 0, 0, 0, 3], to=L, L=L))
    burst += [_ok(0, z, to=3, L=1, x=1, ballot=(2, 3)), _ok(1, z, to=3, L=1, x=1, ballot=(2, 3))]
    res = both(n, [("lead", leads), ("replies", burst)])
    assert sorted(r[0] for r in res[1][1] if r[0] >= 3) == [3, 3, 3, 3, 4, 4]


@pytest.mark.parametrize("size", [1, 63, 64, 65, 3 * 4096 + 1])
def test_burst_sizes(size):
    # 3 * 4096 + 1 crosses the sort's tile and every workgroup boundary; the answers of an instance are far apart in the burst
    n = 5
    inst = (size + 2) // 3
    per = (inst + n - 1) // n
    leads = [(j % n, j // n, j % n, 0, -1 if j % 3 else j % 4, 1, j, int(j % 11 == 0)) for j in range(inst)]
    burst = []
    for q in range(3):
        for j in range(inst):
            w = [0] * n
            if j % 7 == 0 and q == 1:
                w[(j + 1) % n] = 1 + j % 3
            burst.append(_ok((j % n + 1 + q) % n, w, to=j % n, L=j % n, x=j // n, seq=int(j % 13 == 0 and q == 0)))
    res = both(n, [("lead", leads), ("replies", burst[:size])], num_instances=per + 1)
    assert len(res[1][1]) == size


def test_a_burst_that_takes_the_block_count_scan_past_its_first_step():
    # k_lr_count -> k_lr_bscan -> k_lr_compact with more blocks than the one workgroup of k_lr_bscan scans in a step (256
    # blocks of LR_BLOCK = 1024 messages): 256 * 1024 + 1024 + 1 messages.  The burst is one burst of 64 messages again and
    # again, each copy on instances of its own (Noops, so a copy's answers do not depend on its instance numbers): the model
    # answers the 64 once, and its answer repeats.  Messages 0 and 63 of the 64 decide, so the first block, the last message
    # of the first step (262 143), the first of the second (262 144) and the one message of the final block all do
    n, B, STEP = 3, 64, 256 * 1024
    m = STEP + 1024 + 1
    leads, burst = [], []
    for k in range(B):
        if k % 4 == 1:                                            # a second answer for the instance before: ignored
            burst.append(burst[-1])
            continue
        j = len(leads)
        L, x = j % n, j // n
        leads.append((L, x, L, 0, -1, 1, j, int(j % 5 == 0)))
        w = [0] * n
        if j % 7 == 0:
            w[(L + 1) % n] = 1 + j % 3                            # one more dependency than the leader named: the slow path
        burst.append(_ok((L + 1 + j % 2) % n, w, to=L, L=L, x=x, seq=int(j % 13 == 0)))
    per = (len(leads) + n - 1) // n                               # instance numbers a copy takes of every leader
    copies = (m + B - 1) // B
    model = M.LeaderModel(n, 4, per)
    want = S.run_model(model, [("lead", leads), ("replies", burst)])
    assert want[0][0] == 0 and want[1][0] == 0
    rows = want[1][1]
    assert rows[0][0] in (3, 4, 5) and rows[63][0] in (3, 4, 5) and sorted(set(r[0] for r in rows))[0] < 3
    assert (m - 1) % B == 0 and (STEP - 1) % B == 63

    def tiled(col, shift=0, upto=None):
        a = np.tile(np.asarray(col, np.int32), (copies,) + (1,) * (np.ndim(col) - 1))
        if shift:
            a = a + np.repeat(np.arange(copies, dtype=np.int32) * shift, len(col))
        return a[:upto]

    e = ctx(n, num_instances=per * copies)
    lc = list(zip(*leads))
    st, deps, dend = e.lead(tiled(lc[0]), tiled(lc[1], per), tiled(lc[2]), tiled(lc[3]), tiled(lc[4]),
                            tiled(lc[5]).astype(np.uint8), tiled(lc[6]), tiled(lc[7]).astype(np.uint8))
    assert st == 0
    np.testing.assert_array_equal(deps, tiled([d[0] for d in want[0][1]]))
    np.testing.assert_array_equal(dend, tiled([d[1] for d in want[0][1]]))
    a = S.burst_arrays(n, burst)
    st, outcome, oseq, odeps, oend, otr, dec = e.leader_replies(*[tiled(c, per if k == 3 else 0, m) for k, c in enumerate(a)])
    assert st == 0
    for got, k in [(outcome, 0), (oseq, 1), (odeps, 2), (oend, 3), (otr, 4)]:
        np.testing.assert_array_equal(got, tiled([r[k] for r in rows], 0, m))
    expect = np.flatnonzero(np.isin(outcome, [3, 4, 5]))
    np.testing.assert_array_equal(dec, expect)                    # (its length is num_decided)
    assert {0, STEP - 1, STEP, m - 1} <= set(expect.tolist()) and len(expect) < m
    e.close()


def test_a_run_of_200_resent_answers():
    n, z = 5, [0] * 5
    burst = [_ok(1 + (j % 2), [0, j % 3, 0, 0, 0]) for j in range(199)] + [_ok(3, z), _ok(4, z)]
    res = both(n, [("lead", [(0, 0, 0, 0, 0, 1, 5, 0)]), ("replies", burst)])
    assert res[1][2] == [199]


def test_empty_burst_and_empty_lead():
    e = ctx(5)
    z = np.zeros(0, np.int32)
    st, outcome, _, _, _, _, dec = e.leader_replies(z, z, z, z, z, z, z)
    assert st == 0 and len(outcome) == 0 and len(dec) == 0
    assert e.lead(z, z, z, z, z, z.astype(np.uint8), z)[0] == 0
    e.close()


def test_without_the_flag_the_three_calls_are_refused():
    import torch

    e = ctx(5, leader_state=False)
    one = np.zeros(1, np.int32)
    assert e.lead(one, one, one, one, one, one.astype(np.uint8), one)[0] == M.EINVAL
    assert e.leader_replies(one, one, one, one, one, one, one)[0] == M.EINVAL
    t = torch.zeros(8, dtype=torch.int32, device="cuda")
    from frankenpaxos_amd import FpxError

    with pytest.raises(FpxError):
        e.leader_replies_dev(t[:1], t[:1], t[:1], t[:1], t[:1], t[:1], t[:1], t[:1], t[:5], t[:1])
    with pytest.raises(FpxError):
        e.read_leader_state(0, 0, 0)
    assert e.read_cmdlog(0, 0, 0)[0] == 0
    e.close()
    from frankenpaxos_amd.epaxos import EPaxos

    with pytest.raises(FpxError):
        EPaxos(5, 4, num_instances=0, leader_state=True)


def test_every_einval_case_leaves_state_and_outputs_untouched():
    n, z = 5, [0] * 5
    ops = [("lead", [(0, 2, 0, 0, 1, 1, 7, 0), (1, 0, 1, 0, 1, 0, 8, 0)]), ("replies", [_ok(1, z, x=2)])]
    good = _ok(2, z, x=2)
    bad_replies = [
        (4, 0, 0, 2, 0, 0, 1, 0, z, 0), (-1, 0, 0, 2, 0, 0, 1, 0, z, 0),               # an unknown kind
        _ok(2, z, to=5, x=2), _ok(2, z, to=-1, x=2), _ok(5, z, x=2), _ok(-1, z, x=2),  # to / replica_index outside 0..n-1
        _ok(2, z, x=64), _ok(2, z, x=-1), _ok(2, z, L=5, x=2),                          # an instance outside the log
        _ok(2, [0, -1, 0, 0, 0], x=2),                                                  # a negative watermark
        _ok(2, [2, 0, 0, 0, 0], x=2, end=3), _ok(2, [1, 0, 0, 0, 0], x=2, end=5), _ok(2, z, x=2, end=-1),   # explicit ids
        _ok(2, z, x=2, ballot=(0, 5)), _ok(2, z, x=2, ballot=(1 << 27, 0)),
        (M.NACK, 0, 0, 2, -1, 0, 1, 0, z, 0), (M.ACCEPT_OK, 0, 0, 2, 0, 0, 7, 0, z, 0),
    ]
    bad_leads = [(5, 0, 0, 0, 0, 1, 1, 0), (0, 64, 0, 0, 0, 1, 1, 0), (0, 3, 5, 0, 0, 1, 1, 0), (0, 3, -1, 0, 0, 1, 1, 0),
                 (0, 3, 0, 0, 4, 1, 1, 0), (0, 3, 0, 0, -2, 1, 1, 0), (0, 3, 0, -1, 0, 1, 1, 0), (0, 3, 0, 1, 0, 1, 2, 0)]
    e, model = ctx(n), M.LeaderModel(n, 4, 64)
    assert S.run_gpu(e, ops) == S.run_model(model, ops)
    probe = ops + [("replies", [good] + [_ok(3, z, x=5, L=1)]), ("lead", [(0, 3, 0, 0, 0, 1, 1, 0), (1, 5, 1, 0, 0, 1, 1, 0)])]
    before = S.gpu_state(e, probe)
    assert before == S.model_state(model, probe)
    for bad in bad_replies:
        burst = [good, bad, _ok(3, z, x=2)]
        st, outcome, oseq, odeps, oend, otr, dec = e.leader_replies(*S.burst_arrays(n, burst))
        assert st == M.EINVAL and model.replies(burst)[0] == M.EINVAL, bad
        assert (outcome == -9).all() and (oseq == -9).all() and (odeps == -9).all() and (oend == -9).all() and (otr == -9).all()
        assert len(dec) == 0
    for bad in bad_leads:
        msgs = [(0, 3, 0, 0, 0, 1, 1, 0), bad]                      # (the last one repeats an instance of the call)
        assert S.run_gpu_op(e, ("lead", msgs)) == (M.EINVAL, None) and model.lead(msgs)[0] == M.EINVAL, bad
    assert S.gpu_state(e, probe) == before
    # and the context still works
    tail = [("replies", [good, _ok(3, z, x=2)])]
    assert S.run_gpu(e, tail) == S.run_model(model, tail)
    e.close()


def test_a_commit_leaves_the_conflict_index_as_lead_left_it():
    # commit -> updateConflictIndex (:828) repeats the put of transitionToPreAcceptPhase (:694); TopOne.put is a maximum
    n, z = 5, [0] * 5
    e = ctx(n)
    assert e.lead([0, 0], [0, 1], [0, 0], [0, 0], [2, 2], [1, 0], [5, 6])[0] == 0
    before = [e.read_index(r, 2) for r in range(n)]
    assert before[0][0].tolist() == [2, 0, 0, 0, 0] and before[0][1].tolist() == [1, 0, 0, 0, 0]
    burst = [_ok(q, z, x=0) for q in (1, 2, 3)] + [_ok(1, [1, 0, 0, 0, 0], x=1), _ok(2, [1, 0, 0, 1, 0], x=1), _ok(3, [1, 0, 0, 0, 0], x=1)]
    burst += [(M.ACCEPT_OK, 0, 0, 1, 0, 0, q, 0, z, 0) for q in (1, 2)]
    st, outcome = e.leader_replies(*S.burst_arrays(n, burst))[:2]
    assert st == 0 and outcome.tolist() == [1, 2, 3, 1, 2, 4, 1, 5]
    after = [e.read_index(r, 2) for r in range(n)]
    for a, b in zip(before, after):
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert e.read_cmdlog(0, 0, 0)[0] == 4 and e.read_cmdlog(0, 0, 1)[0] == 4
    e.close()


def test_the_device_form_equals_the_host_form():
    import torch

    n = 5
    ops = S.make_stream(2, n)
    lead_ops = [op for op in ops if op[0] != "replies"]
    burst = next(op for op in ops if op[0] == "replies")[1]
    upto = ops.index(("replies", burst))
    host, dev = ctx(n), ctx(n)
    S.run_gpu(host, ops[:upto]), S.run_gpu(dev, ops[:upto])
    a = S.burst_arrays(n, burst)
    want = host.leader_replies(*a)
    m = len(burst)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(5)]
    odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
    nd = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.leader_replies_dev(*[T(x) for x in a], outcome=outs[0], out_seq=outs[1], out_deps=odeps, out_values_end=outs[2],
                           out_triple=outs[3], decided_index=outs[4], num_decided=nd)
    assert dev.sync() == want[0]
    k = int(nd.item())
    assert k == len(want[6]) and outs[4][:k].cpu().numpy().tolist() == want[6].tolist()
    for got, w in zip([outs[0], outs[1], odeps, outs[2], outs[3]], want[1:6]):
        assert (got.cpu().numpy() == w).all()
    probe = ops[:upto + 1]
    assert S.gpu_state(dev, probe) == S.gpu_state(host, probe)
    assert lead_ops
    host.close(), dev.close()


def test_cross_route_the_tick_and_lead_plus_replies_decide_alike():
    """Context A: fpx_epx_preaccept (the oracle-verified all-in-one-process tick) with the rank rows one global event order
    implies.  Context B: the same events replayed with fpx_epx_lead / fpx_epx_handle_preaccept, one message per call, then
    every PreAcceptOk, shuffled, through ONE fpx_epx_leader_replies."""
    from frankenpaxos_amd.epaxos import EPaxos

    n, num_keys, m = 5, 16, 48
    rng = np.random.default_rng(7)
    leader = rng.integers(0, n, m).astype(np.int32)
    number = np.zeros(m, np.int32)
    key = rng.integers(0, num_keys, m).astype(np.int32)
    is_set = rng.integers(0, 2, m).astype(np.uint8)
    tid = (np.arange(m) + 100).astype(np.int32)
    peers = [rng.permutation([r for r in range(n) if r != int(leader[i])])[:n - 2] for i in range(m)]
    mask = np.array([sum(1 << int(r) for r in p) for p in peers], np.uint8)
    # a global event order: every command is led first, then delivered to its n - 2 thrifty peers
    events, pending = [], [[("lead", i)] + [("deliver", i, int(r)) for r in rng.permutation(peers[i])] for i in rng.permutation(m)]
    nxt = [0] * n
    while pending:
        j = int(rng.integers(0, len(pending)))
        ev = pending[j].pop(0)
        if ev[0] == "lead":                                      # a leader numbers its instances in the order it leads them
            number[ev[1]] = nxt[int(leader[ev[1]])]
            nxt[int(leader[ev[1]])] += 1
        events.append(ev)
        if not pending[j]:
            pending.pop(j)
    rank = np.zeros((n, m), np.int32)
    for r in range(n):
        seq = [ev[1] for ev in events if (ev[0] == "lead" and int(leader[ev[1]]) == r) or (ev[0] == "deliver" and ev[2] == r)]
        rest = [i for i in range(m) if i not in set(seq)]
        for pos, i in enumerate(seq + rest):
            rank[r, i] = pos
    A = EPaxos(n, num_keys, num_instances=m)
    st, fast, deps, ldeps, own = A.preaccept(leader, number, key, is_set, mask, rank, triple_id=tid)
    assert st == 0

    B = EPaxos(n, num_keys, num_instances=m, leader_state=True)
    lead_deps, burst = {}, []
    one = lambda v: np.asarray([v], np.int32)
    for ev in events:
        i = ev[1]
        L, x = int(leader[i]), int(number[i])
        if ev[0] == "lead":
            st, d, de = B.lead(one(L), one(x), one(L), one(0), one(key[i]), [is_set[i]], one(tid[i]))
            assert st == 0
            lead_deps[i] = (d[0].copy(), int(de[0]))
        else:
            r = ev[2]
            d, de = lead_deps[i]
            res = B.handle_preaccept(one(L), one(x), one(0), one(L), one(key[i]), [is_set[i]], one(tid[i]), d[None, :], one(de),
                                     [1 << r])
            assert res[0] == 0 and res[1][0] == 1 << r
            burst.append(_ok(r, res[6][0, r].tolist(), to=L, L=L, x=x, ballot=(0, L), end=int(res[7][0, r])))
    burst = [burst[j] for j in rng.permutation(len(burst))]
    st, outcome, oseq, odeps, oend, otr, dec = B.leader_replies(*S.burst_arrays(n, burst))
    assert st == 0 and len(dec) == m
    seen = set()
    for j in dec:
        L, x = burst[j][2], burst[j][3]
        i = next(k for k in range(m) if int(leader[k]) == L and int(number[k]) == x)
        seen.add(i)
        assert int(outcome[j]) == (M.FAST_COMMIT if fast[i] else M.ACCEPT), i
        assert odeps[j].tolist() == deps[i].tolist() and int(oend[j]) == int(own[i, 0]) and int(otr[j]) == int(tid[i]), i
        assert lead_deps[i][0].tolist() == ldeps[i].tolist() and lead_deps[i][1] == int(own[i, 1]), i
        a, b = A.read_cmdlog(L, L, x), B.read_cmdlog(L, L, x)
        if fast[i]:                                               # CommittedEntry(the agreed triple) at the leader, both routes
            assert a[:4] == b[:4] == (4, -1, -1, int(tid[i]))
            da, db = A.read_cmdlog_deps(L, L, x), B.read_cmdlog_deps(L, L, x)
            assert da[0].tolist() == db[0].tolist() and da[1] == db[1]
        else:                                                     # the tick stops before the Accept phase; B has entered it
            assert a[:4] == (2, L, L, int(tid[i])) and b[:4] == (3, L, L, int(tid[i]))
            assert B.read_cmdlog_deps(L, L, x)[0].tolist() == deps[i].tolist()
    assert seen == set(range(m)) and 0 < int(fast.sum()) < m
    A.close(), B.close()


def test_agreement_that_holds_only_through_the_own_column_equivalence():
    # instance (0, 4): a cover of 4 and a cover of 5 on column 0 are one set (dependencies.subtractOne, :582); raw
    # watermarks would disagree and send the instance down the slow path
    n = 5
    ops = [("lead", [(0, 4, 0, 0, 0, 1, 9, 0)]),
           ("replies", [_ok(1, [4, 0, 2, 0, 0], x=4), _ok(2, [5, 0, 2, 0, 0], x=4), _ok(3, [4, 0, 2, 0, 0], x=4)])]
    res = both(n, ops)
    assert res[1][1][2] == (M.FAST_COMMIT, 0, [4, 0, 2, 0, 0], 0, 9)
    # and a union is taken on covers: explicit ids above the instance from one sender, a plain cover from another
    ops = [("lead", [(0, 4, 0, 0, 0, 1, 9, 0)]),
           ("replies", [_ok(1, [4, 0, 0, 0, 0], x=4, end=8), _ok(2, [5, 0, 0, 0, 0], x=4), _ok(3, [2, 1, 0, 0, 0], x=4)])]
    res = both(n, ops)
    assert res[1][1][2] == (M.ACCEPT, 0, [4, 1, 0, 0, 0], 8, 9)
