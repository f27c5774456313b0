"""Originating an instance's recovery on the device (fpx_epx_recover, fpx_epx_recovery_replies[_dev], fpx_epx_lead_accept with
FPX_EPX_F_RECOVERY) against tests/epaxos_recovery_model.py, bit for bit on every output; the leader state, the command log
and the conflict index are compared through fpx_epx_read_leader_state / fpx_epx_read_recovery_state /
fpx_epx_read_cmdlog[_deps] / fpx_epx_read_index."""
import ctypes as C

import numpy as np
import pytest

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as LS
from tests import epaxos_recovery_model as R
from tests import epaxos_recovery_streams as S

pytestmark = pytest.mark.gpu
NK, NI = 4, 64


def ctx(n, recovery=True, leader_state=True, num_instances=NI):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, NK, num_instances=num_instances, leader_state=leader_state, recovery=recovery)


def both(n, ops, num_instances=NI):
    e, model = ctx(n, num_instances=num_instances), R.RecoveryModel(n, NK, num_instances)
    for k, op in enumerate(ops):
        got, want = S.run_gpu_op(e, op), S.run_op(model, op)
        assert got == want, (k, op[0])
    same_state(S.gpu_state(e, ops), S.model_state(model, ops))
    e.close()


def same_state(got, want):
    for cell in want[0]:
        assert got[0][cell] == want[0][cell], cell
    assert got == want


@pytest.mark.parametrize("as_intended", [False, True])
@pytest.mark.parametrize("n", [3, 5, 7])
def test_the_generators_streams(n, as_intended):
    # every outcome of recover and recovery_replies, every entry state, stale / duplicate / replaced / too-large PrepareOks, a
    # Nack and a peer's Prepare mid-recovery, two recoveries at one replica in a call (tests/test_epaxos_recovery_cpu.py
    # asserts the census)
    both(n, S.make_stream(1, n, as_intended)[0])


def cut(ops, how):
    out = []
    for op in ops:
        if op[0] != "prepare_oks":
            out.append(op)
        elif how == "two":
            h = len(op[1]) // 2
            out += [("prepare_oks", op[1][:h], op[2]), ("prepare_oks", op[1][h:], op[2])]
        else:
            out += [("prepare_oks", [msg], op[2]) for msg in op[1]]
    return out


@pytest.mark.parametrize("n", [3, 5, 7])
def test_a_burst_cut_in_two_and_one_message_per_call(n):
    ops = S.make_stream(2, n, True)[0]
    whole = ctx(n)
    rows = {"whole": [], "two": [], "each": []}
    for op in ops:
        res = S.run_gpu_op(whole, op)
        if op[0] == "prepare_oks":
            rows["whole"] += res[1]
    want_state = S.gpu_state(whole, ops)
    whole.close()
    for how in ("two", "each"):
        e = ctx(n)
        for op in cut(ops, how):
            res = S.run_gpu_op(e, op)
            if op[0] == "prepare_oks" and op[1]:
                rows[how] += res[1]
        assert rows[how] == rows["whole"], how
        assert S.gpu_state(e, ops) == want_state, how
        e.close()


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1025, 4097])
def test_burst_lengths(m):
    # around the 256-thread blocks, LR_BLOCK = 1024 and more than one sort tile; a handful of cells, so a run is hundreds of
    # messages long; n = 7 decides at four responses, so senders repeat and replace before a decision
    n = 7
    for as_intended in (False, True):
        rec, burst = S.random_burst(m, n, m)
        both(n, [rec, ("prepare_oks", burst, as_intended)])


@pytest.mark.parametrize("n", [3, 5, 7])
def test_a_call_of_600_recoveries_ranks_every_replica_in_one_launch(n):
    # k_lr_bscan scans the n rows of `rank` in one launch, a workgroup per row, 256 flags a step: a call of 600 is three steps
    # per row with a ragged last one.  at[] is uneven -- replica 0 takes most of the call (more than two steps of ones),
    # replica 1 nothing at all (a row of zeros, total 0), the others a few each -- so every row has another total and long
    # stretches of zeros.  Some instances are committed, pre-accepted or were already recovered by an earlier call when the
    # call meets them (a second recovery of an instance takes a ballot above the first; the SAME instance twice in one call
    # is FPX_EINVAL by contract, which the call before the last holds against the model on rows of this length).
    import random

    m, ni = 600, 256
    rng = random.Random(100 + n)
    insts = rng.sample([(L, x) for L in range(n) for x in range(ni)], m)
    ats = rng.choices(range(n), [20, 0] + list(range(1, n - 1)), k=m)
    per_row = [ats.count(r) for r in range(n)]
    assert per_row[0] > 512 - 256 and per_row[1] == 0 and len(set(per_row)) == n and all(c > 0 for c in per_row[2:])
    z, ops = [0] * n, []
    for k, (inst, at) in enumerate(zip(insts, ats)):
        if k % 7 == 0:
            ops.append(("commit", inst, 3000 + k, z, 0, at, k % NK, k & 1))
        elif k % 11 == 0:
            ops.append(("preaccept", inst, (0, inst[0]), k % NK, k & 1, 3000 + k, z, 0, at))
    call = [(i[0], i[1], at) for i, at in zip(insts, ats)]
    ops.append(("recover", call[1::5]))                                # (some of them committed: k = 21, 56, ..)
    ops.append(("recover", call + [call[300]]))                        # FPX_EINVAL: nothing moves
    ops.append(("recover", call))
    e, model = ctx(n, num_instances=ni), R.RecoveryModel(n, NK, ni)
    res = [(S.run_gpu_op(e, op), S.run_op(model, op)) for op in ops]
    for k, (got, want) in enumerate(res):
        assert got == want, (k, ops[k][0])
    assert res[-2][0] == (R.EINVAL, None) and res[-1][0][0] == 0
    rows = res[-1][0][1]                                               # (outcome, ballot ordering, status, vote, triple)
    assert {r[0] for r in rows} == {R.RV_PREPARING, R.RV_COMMITTED} and {r[2] for r in rows} >= {-1, 0, 2}
    for r in range(n):                                                 # the ranks of a row are 0 .. its total - 1, in order
        mine = [row[1] for row, at in zip(rows, ats) if at == r]
        assert mine == list(range(mine[0], mine[0] + per_row[r])) if mine else per_row[r] == 0
    same_state(S.gpu_state(e, ops), S.model_state(model, ops))
    e.close()


def test_the_device_form_on_the_contexts_stream():
    import torch

    n = 5
    ops = S.make_stream(3, n, True)[0]
    model = R.RecoveryModel(n, NK, NI)
    results = [S.run_op(model, op) for op in ops]
    upto = next(k for k, op in enumerate(ops) if op[0] == "prepare_oks" and results[k][0] == R.EFATAL)
    burst = ops[upto][1]
    host, dev = ctx(n), ctx(n)
    for op in ops[:upto]:
        assert S.run_gpu_op(host, op) == S.run_gpu_op(dev, op)
    a = S.prepare_ok_arrays(n, burst)
    want = host.recovery_replies(*a[:10], a[10], a[11], a[12], as_intended=True)
    assert want[0] == R.EFATAL                                     # (the stream holds a PrepareOk above the state's ballot)
    m = len(burst)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs = [torch.full((m,), -9, dtype=torch.int32, device="cuda") for _ in range(7)]
    odeps = torch.full((m, n), -9, dtype=torch.int32, device="cuda")
    nd = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.recovery_replies_dev(*[T(x) for x in a], as_intended=True, outcome=outs[0], out_source=outs[1], out_triple=outs[2],
                             out_ballot=outs[3], out_seq=outs[4], out_deps=odeps, out_values_end=outs[5], decided_index=outs[6],
                             num_decided=nd)
    assert dev.sync() == want[0]
    k = int(nd.item())
    assert k == len(want[8]) > 0 and outs[6][:k].cpu().numpy().tolist() == want[8].tolist()
    for got, w in zip([outs[0], outs[1], outs[2], outs[3], outs[4], odeps, outs[5]], want[1:8]):
        assert (got.cpu().numpy() == w).all()
    assert S.gpu_state(dev, ops[:upto + 1]) == S.gpu_state(host, ops[:upto + 1])
    # an empty burst: num_decided is written, nothing else happens
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    dev.recovery_replies_dev(*[z] * 13, num_decided=nd)
    assert dev.sync() == 0 and int(nd.item()) == 0
    host.close(), dev.close()


# ---- a recovery end to end between two contexts: A hosts replica 0, B stands for the remote peers ---------------------------
def _inbox(e, model, msgs):
    """msgs: (kind, to, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, watermarks, values_end) into
    e's fpx_epx_replica_inbox and, one at a time, into the model; returns the GPU's reply arrays"""
    n = e.n
    cols = [np.asarray(c, np.int32) for c in zip(*[m[:9] for m in msgs])]
    deps = np.asarray([m[9] for m in msgs], np.int32).reshape(len(msgs), n)
    dend = np.asarray([m[10] for m in msgs], np.int32)
    st, outcome, ob, os_, odeps, oend, otr = e.replica_inbox(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], cols[6],
                                                            cols[7].astype(np.uint8), cols[8], deps, dend)
    assert st == 0
    for (kind, to, L, x, bo, br, key, is_set, tid, w, end) in msgs:
        inst = (L, x)
        if kind == 0:
            model.peer_preaccept(inst, (bo, br), key, bool(is_set), tid, LS.decode_deps(n, inst, w, end), [to])
        elif kind == 1:
            # handleAccept alone (:1476-1511): the entry is taken in with the message's dependencies
            from oracle import epaxos_sets as ES
            rep = model.replicas[to]
            model._yield_to(to, inst, (bo, br))
            rep.largest_ballot = max(rep.largest_ballot, (bo, br))
            rep.cmd_log[inst] = ES.Entry(ES.ACCEPTED, (bo, br), (bo, br), tid, LS.decode_deps(n, inst, w, end))
            if key >= 0:
                rep.index_put(key, bool(is_set), inst)
        elif kind == 2:
            model.peer_commit(inst, tid, LS.decode_deps(n, inst, w, end), [to], key, bool(is_set))
        else:
            model.peer_prepare(inst, (bo, br), [to])
    return outcome, ob, os_, odeps, oend, otr


def _hosted_state(e, model, hosted, inst, keys):
    """the cells of `inst` at the replicas this context hosts, and those replicas' index and largestBallot, GPU == model"""
    ops = [("recover", [(inst[0], inst[1], r) for r in hosted])]
    g, w = S.gpu_state(e, ops), S.model_state(model, ops)
    assert g[0] == w[0]
    for r in hosted:
        assert g[1][r] == w[1][r]
        for k in keys:
            gg, ss = e.read_index(r, k)
            assert (gg.tolist(), ss.tolist()) == (model.replicas[r].gets[k], model.replicas[r].sets[k])


@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("kind", ["noop", "pre_accept", "accept_popular", "accept_accepted"])
def test_a_recovery_end_to_end_between_two_contexts(n, kind):
    f = (n - 1) // 2
    inst, key, tid, z = (1, 3), 2, 41, [0] * n
    A, B, model = ctx(n), ctx(n, recovery=False), R.RecoveryModel(n, NK, NI)
    peers = list(range(1, n))
    quorum = [q for q in peers if q != inst[0]][:f] if n > 3 else [2]      # (not the instance's dead leader, replica 1)
    # ---- what the dead leader left behind at the peers
    if kind in ("pre_accept", "accept_popular"):
        left = quorum if kind == "accept_popular" else quorum[:1]
        _inbox(B, model, [(0, q, inst[0], inst[1], 0, inst[0], key, 1, tid, z, 0) for q in left])
    elif kind == "accept_accepted":
        _inbox(B, model, [(1, quorum[0], inst[0], inst[1], 0, inst[0], key, 1, tid, [0] * (n - 1) + [1], 0)])
    # ---- recover on A, the Prepare into B, the PrepareOks into A
    rec = ("recover", [(inst[0], inst[1], 0)])
    got = S.run_gpu_op(A, rec)
    assert got == S.run_op(model, rec) and got[1][0][0] == R.RV_PREPARING
    bo = got[1][0][1]
    outcome, ob, os_, odeps, oend, otr = _inbox(B, model, [(3, q, inst[0], inst[1], bo, 0, -1, 0, -1, z, 0) for q in quorum])
    assert (outcome == 6).all()                                      # FPX_EPX_RI_PREPARE_OK
    oks = []
    for j, q in enumerate(quorum):
        vb = int(ob[j])
        oks.append((0, inst[0], inst[1], bo, 0, q, int(os_[j]), -1 if vb < 0 else vb >> 3, -1 if vb < 0 else vb & 7, int(otr[j]),
                    0, [max(int(v), 0) for v in odeps[j]], int(oend[j])))
    op = ("prepare_oks", oks, True)
    got = S.run_gpu_op(A, op)
    assert got == S.run_op(model, op)
    want = {"noop": R.RC_PRE_ACCEPT_NOOP, "pre_accept": R.RC_PRE_ACCEPT if n > 3 else R.RC_ACCEPT, "accept_popular": R.RC_ACCEPT,
            "accept_accepted": R.RC_ACCEPT}[kind]
    assert got[2] == [len(oks) - 1] and got[1][-1][0] == want
    (_, src, dtid, dballot, dseq, dw, dend) = got[1][-1]
    assert dballot == bo * 8
    _hosted_state(A, model, [0], inst, [key])
    # ---- the decision applied, the PreAccept / Accept into B, the Oks into A, the Commit
    ckey, cset, ctid = (-1, 0, S.NOOP_TRIPLE) if want == R.RC_PRE_ACCEPT_NOOP else (key, 1, dtid)
    if want == R.RC_ACCEPT:
        op = ("lead_accept", [(inst[0], inst[1], 0, bo, ckey, cset, ctid, dseq, dw, dend)])
        assert S.run_gpu_op(A, op) == S.run_op(model, op) == (0,)
        aw, aend, aseq = dw, dend, dseq
    else:
        op = ("lead", [(inst[0], inst[1], 0, bo, ckey, cset, ctid, 1)])
        got = S.run_gpu_op(A, op)
        assert got == S.run_op(model, op) and got[0] == 0
        pw, pend = got[1][0]
        outcome, ob, os_, odeps, oend, otr = _inbox(B, model, [(0, q, inst[0], inst[1], bo, 0, ckey, cset, ctid, pw, pend)
                                                             for q in quorum])
        assert (outcome == 1).all()                                  # FPX_EPX_RI_PRE_ACCEPT_OK
        op = ("replies", [(M.PRE_ACCEPT_OK, 0, inst[0], inst[1], bo, 0, q, 0, [int(v) for v in odeps[j]], int(oend[j]))
                          for j, q in enumerate(quorum)])
        got = S.run_gpu_op(A, op)
        assert got == S.run_op(model, op) and got[1][-1][0] == M.ACCEPT     # avoidFastPath: the slow path at f + 1
        (_, aseq, aw, aend, _) = got[1][-1]
    _hosted_state(A, model, [0], inst, [key])
    outcome = _inbox(B, model, [(1, q, inst[0], inst[1], bo, 0, ckey, cset, ctid, aw, aend) for q in quorum])[0]
    assert (outcome == 3).all()                                      # FPX_EPX_RI_ACCEPT_OK
    op = ("replies", [(M.ACCEPT_OK, 0, inst[0], inst[1], bo, 0, q, 0, z, 0) for q in quorum])
    got = S.run_gpu_op(A, op)
    assert got == S.run_op(model, op) and got[1][-1][0] == M.SLOW_COMMIT and got[1][-1][4] == ctid
    (_, cseq, cw, cend, _) = got[1][-1]
    assert (cw, cend) == (aw, aend)
    outcome = _inbox(B, model, [(2, q, inst[0], inst[1], 0, 0, ckey, cset, ctid, cw, cend) for q in peers])[0]
    assert (outcome == 5).all()                                      # FPX_EPX_RI_LEARNT
    _hosted_state(A, model, [0], inst, [key])
    _hosted_state(B, model, peers, inst, [key])
    assert A.read_cmdlog(0, *inst)[:4] == (4, -1, -1, ctid) and B.read_cmdlog(peers[-1], *inst)[:4] == (4, -1, -1, ctid)
    A.close(), B.close()


def test_lead_admits_an_entry_whose_ballot_is_the_new_one_with_a_lower_vote():
    # after a recovery the entry at the recovering replica carries the recovery's ballot and the vote it was pre-accepted
    # in; transitionToPreAcceptPhase's checkLe (:672-681) admits it, and the dependencies come from the index
    n = 5
    ops = [("preaccept", (1, 0), (0, 1), 2, 1, 30, [0] * n, 0, 0),           # the index of replica 0 learns (1, 0) under key 2
           ("preaccept", (2, 5), (0, 2), 2, 1, 31, [0] * n, 0, 0),
           ("recover", [(2, 5, 0)]),
           ("prepare_oks", [(0, 2, 5, 1, 0, 1, 0, -1, -1, -1, 0, [0] * n, 0), (0, 2, 5, 1, 0, 3, 0, -1, -1, -1, 0, [0] * n, 0)], False),
           ("lead", [(2, 5, 0, 1, 2, 1, 31, 1)])]
    e, model = ctx(n), R.RecoveryModel(n, NK, NI)
    res = [(S.run_gpu_op(e, op), S.run_op(model, op)) for op in ops]
    assert all(g == w for g, w in res)
    assert e.read_cmdlog(0, 2, 5)[:4] == (2, 8, 8, 31)                       # PreAccepted in (1, 0), voted there now
    assert res[2][0][1][0] == (R.RV_PREPARING, 1, 2, 2 * 1 + 0 * 8, 31) and res[3][0][1][1][0] == R.RC_PRE_ACCEPT
    assert res[4][0] == (0, [([0, 1, 5, 0, 0], 0)])                          # from the index of replica 0; never the instance itself
    assert S.gpu_state(e, ops) == S.model_state(model, ops)
    e.close()


def test_without_the_flag_the_new_calls_are_refused_and_the_rest_is_as_before():
    import torch
    from frankenpaxos_amd import FpxError
    from frankenpaxos_amd.epaxos import EPaxos

    n = 5
    e = ctx(n, recovery=False)
    one, z = np.zeros(1, np.int32), np.zeros((1, n), np.int32)
    assert e.recover(one, one, one)[0] == R.EINVAL
    assert e.recovery_replies(one, one, one, one, one, one, one, one - 1, one - 1, one)[0] == R.EINVAL
    assert e.lead_accept(one, one, one, one, one, one.astype(np.uint8), one, one, z) == R.EINVAL
    t = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(FpxError):
        e.recovery_replies_dev(*[t[:1]] * 11, t[:5], t[:1])
    with pytest.raises(FpxError):
        e.read_recovery_state(0, 0, 0)
    with pytest.raises(FpxError):                                             # the flag needs FPX_EPX_F_LEADER_STATE
        EPaxos(n, NK, num_instances=NI, leader_state=False, recovery=True)
    # fpx_epx_info and the leader readbacks: a context with the flag and one without show the same
    f = ctx(n)
    ops = LS.make_stream(1, n)
    assert LS.run_gpu(e, ops) == LS.run_gpu(f, ops)
    info = []
    for c in (e, f):
        v = [C.c_int32(-1) for _ in range(3)]
        assert c.L.fpx_epx_info(c._h, *[C.byref(x) for x in v]) == 0
        info.append(tuple(x.value for x in v))
    assert info[0] == info[1] == (n, NK, NI)
    assert LS.gpu_state(e, ops) == LS.gpu_state(f, ops)
    e.close(), f.close()


@pytest.mark.parametrize("n", [3, 5, 7])
def test_with_the_flag_the_leader_streams_are_bit_identical(n):
    ops = LS.make_stream(2, n)
    model = M.LeaderModel(n, NK, NI)
    want = LS.run_model(model, ops)
    e = ctx(n)
    assert LS.run_gpu(e, ops) == want
    assert LS.gpu_state(e, ops) == LS.model_state(model, ops)
    e.close()


def test_every_einval_case_leaves_state_and_outputs_untouched():
    n, z = 5, [0] * 5
    ops = [("preaccept", (1, 2), (0, 1), 1, 1, 9, z, 0, 0), ("recover", [(1, 2, 0), (2, 0, 3)])]
    e, model = ctx(n), R.RecoveryModel(n, NK, NI)
    for op in ops:
        assert S.run_gpu_op(e, op) == S.run_op(model, op)
    ok = lambda **kw: tuple(kw.get(k, d) for k, d in [("to", 0), ("L", 1), ("x", 2), ("bo", 1), ("br", 0), ("q", 1), ("s", 2),
                                                      ("vo", 0), ("vr", 1), ("t", 9), ("seq", 0), ("w", z), ("end", 0)])
    good = ok()
    bad_oks = [ok(to=5), ok(to=-1), ok(L=5), ok(x=NI), ok(x=-1), ok(bo=-1), ok(bo=1 << 27), ok(br=5), ok(q=5), ok(q=-1),
               ok(s=1), ok(s=4), ok(s=-1), ok(vo=-1, vr=0), ok(vo=0, vr=-1), ok(vo=1 << 27), ok(vr=5), ok(vo=-2, vr=-2),
               ok(w=[0, -1, 0, 0, 0]), ok(w=[0, 1, 0, 0, 0], end=4), ok(end=3), ok(w=[0, 2, 0, 0, 0], end=-1), ok(s=3, w=[-1] * 5)]
    probe = ops + [("prepare_oks", [good, ok(to=3, L=2, x=0, br=3)], False)]
    before = S.gpu_state(e, probe)
    assert before == S.model_state(model, probe)
    for bad in bad_oks:
        burst = [good, bad, ok(q=2)]
        a = S.prepare_ok_arrays(n, burst)
        res = e.recovery_replies(*a[:10], a[10], a[11], a[12])
        assert res[0] == R.EINVAL and model.prepare_oks(burst)[0] == R.EINVAL, bad
        assert all((x == -9).all() for x in res[1:8]) and len(res[8]) == 0, bad
    assert ok(s=0, w=[-1] * 5)[6] == 0                                # (dependencies of a status-0 message are not read)
    bad_recovers = [(5, 0, 0), (0, NI, 0), (0, -1, 0), (0, 3, 5), (0, 3, -1), (3, 3, 1)]
    for bad in bad_recovers:
        msgs = [(3, 3, 0), bad]                                       # (the last one repeats an instance of the call)
        assert S.run_gpu_op(e, ("recover", msgs)) == (R.EINVAL, None) and model.recover(msgs)[0] == R.EINVAL, bad
    la = lambda **kw: tuple(kw.get(k, d) for k, d in [("L", 3), ("x", 3), ("at", 0), ("bo", 9), ("key", 0), ("set", 1), ("t", 5),
                                                      ("seq", 0), ("w", z), ("end", 0)])
    for bad in [la(L=5), la(x=NI), la(at=5), la(bo=-1), la(bo=1 << 27), la(key=NK), la(key=-2), la(w=[0, -1, 0, 0, 0]),
                la(end=4), la(w=[0, 0, 0, 4, 0], end=7), la(L=4, x=4)]:
        msgs = [la(L=4, x=4), bad]
        assert S.run_gpu_op(e, ("lead_accept", msgs)) == (R.EINVAL,) and model.lead_accept(msgs) == R.EINVAL, bad
    assert S.gpu_state(e, probe + [("recover", [(3, 3, 0), (4, 4, 0)])]) == \
        S.model_state(model, probe + [("recover", [(3, 3, 0), (4, 4, 0)])])
    assert S.gpu_state(e, probe) == before
    # a status-0 message with a malformed row is fine, and the context still works
    tail = [("prepare_oks", [ok(s=0, vo=-1, vr=-1, t=-1, w=[-1] * 5), ok(q=2)], True)]
    for op in tail:
        assert S.run_gpu_op(e, op) == S.run_op(model, op)
    e.close()


def test_an_ordering_that_would_reach_2_to_the_27_is_refused():
    n = 3
    e, model = ctx(n), R.RecoveryModel(n, NK, NI)
    z = [0] * n
    top = (1 << 27) - 2
    op = ("replies", [(M.NACK, 0, 0, 0, top, 1, 1, 0, z, 0)])              # largestBallot(0) = (2^27 - 2, 1)
    assert S.run_gpu_op(e, op) == S.run_op(model, op)
    two = ("recover", [(0, 0, 0), (0, 1, 0)])                              # the second would take ordering 2^27
    assert S.run_gpu_op(e, two) == S.run_op(model, two) == (R.EINVAL, None)
    one = ("recover", [(0, 0, 0), (0, 1, 1)])
    got = S.run_gpu_op(e, one)
    assert got == S.run_op(model, one) and got[1][0][1] == top + 1 and got[1][1][1] == 1
    assert S.gpu_state(e, [one]) == S.model_state(model, [one])
    e.close()
