"""epaxos_recovery_streams.py -- TEST INFRASTRUCTURE ONLY: seeded streams of recovery traffic at hosted EPaxos replicas, the
runners that play a stream on a RecoveryModel or on a GPU context, and a census of the branches a stream reaches.

A stream is a list of the ops of tests/epaxos_leader_streams.py plus
    ("recover", [(leader, number, at), ...])                                                    fpx_epx_recover
    ("prepare_oks", [(to, leader, number, ballot_ordering, ballot_replica, replica_index, status, vote_ordering,
                      vote_replica, triple_id, seq, watermarks, values_end), ...], as_intended)   fpx_epx_recovery_replies
    ("lead_accept", [(leader, number, at, ballot_ordering, key, is_set, triple_id, seq, watermarks, values_end), ...])
The generator drives a RecoveryModel of its own to SHAPE the traffic (which ballot a recovery got, what was decided); what
a stream's results must be is decided by the models under test.
"""
import random

import numpy as np

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as LS
from tests import epaxos_recovery_model as R

NOOP_TRIPLE = 7
ENTRY_STATES = ("unseen", "no_command", "pre_accepted", "accepted", "committed", "fatal")
PATTERNS = ("noop", "pre", "pre_high", "popular", "unpopular", "accepted", "own_column")
EVENTS = ("plain", "stale", "above", "duplicate", "replaced", "own", "late", "prepare_mid", "nack_mid")

# every branch tests/test_epaxos_recovery_cpu.py wants reached (RecoveryModel.census keys)
CENSUS_COMMON = ("recover_unseen", "recover_no_command", "recover_pre_accepted", "recover_accepted", "recover_committed",
                 "recover_fatal", "two_recoveries_at_one_replica", "ok_status_0", "ok_status_2", "ok_status_3", "ok_stale",
                 "ok_duplicate", "ok_replaced", "ok_above", "ok_not_preparing", "nack_while_preparing",
                 "reply_while_preparing", "prepare_while_preparing", "lead_accept")
CENSUS_DECISIONS = {False: ("pre_accept_as_written", "noop_as_written"),
                    True: ("accept_accepted_intended", "accept_popular_intended", "pre_accept_intended", "noop_intended")}


def enc_deps(n, inst, deps):
    return ([-1] * n, 0) if deps is None else LS.encode_deps(n, inst, deps)


def make_stream(seed, n, as_intended, num_keys=4, num_instances=64, rounds=2, per_round=None):
    """rounds x (bring instances into every entry state at their recovering replica, recover them in one call, let a Nack or
    a peer's Prepare hit some, one burst of PrepareOks, the decisions applied, the replies that commit them)"""
    rng = random.Random(seed)
    S = R.RecoveryModel(n, num_keys, num_instances)
    ops, commands, f = [], {NOOP_TRIPLE: (-1, 0)}, (n - 1) // 2
    next_number, triple = [0] * n, [1000]

    def play(op):
        ops.append(op)
        return run_op(S, op)

    def new_triple():
        triple[0] += 1
        commands[triple[0]] = (rng.randrange(num_keys), rng.randrange(2))
        return triple[0]

    per_round = per_round or len(ENTRY_STATES) * 3
    for rnd in range(rounds):
        batch = []
        for j in range(per_round):
            L = rng.randrange(n)
            inst = (L, next_number[L])
            next_number[L] += 1
            at = rng.randrange(n)
            state = ENTRY_STATES[j % len(ENTRY_STATES)]
            pattern = PATTERNS[(j + rnd * 3) % len(PATTERNS)]
            event = EVENTS[(j // 2 + rnd) % len(EVENTS)]
            batch.append((inst, at, state, pattern, event))
        batch_at = batch[0][1]
        batch[1] = (batch[1][0], batch_at) + batch[1][2:]              # two recoveries at one replica in one call
        # ---- the entries the recoveries will meet
        for (inst, at, state, _, _) in batch:
            tid = new_triple()
            key, is_set = commands[tid]
            other = (at + 1) % n
            if state == "no_command":
                play(("prepare", inst, (1, other), at))
            elif state == "pre_accepted":
                play(("preaccept", inst, (0, inst[0]), key, is_set, tid, [0] * n, 0, at))
            elif state in ("accepted", "fatal"):
                bo = S.replicas[at].largest_ballot[0] + (1 + per_round if state == "fatal" else 0)
                play(("lead_accept", [(inst[0], inst[1], at, bo, key, is_set, tid, 0, [0] * n, 0)]))
            elif state == "committed":
                play(("commit", inst, tid, [0] * n, 0, at, key, is_set))
        res = play(("recover", [(i[0], i[1], at) for (i, at, _, _, _) in batch]))[1]
        # ---- mid-recovery events, then each instance's PrepareOks
        per_instance, mid = [], []
        for (inst, at, state, pattern, event), (outcome, bo, own_s, own_v, own_t) in zip(batch, res):
            ballot, peers = (bo, at), [r for r in range(n) if r != at]
            rng.shuffle(peers)
            if event == "prepare_mid":
                mid.append(("prepare", inst, (bo + 1, peers[0]), at))
            elif event == "nack_mid":
                z = [0] * n
                mid.append(("replies", [(M.NACK, at, inst[0], inst[1], bo, at, peers[0], 0, z, 0),
                                        (M.NACK, at, inst[0], inst[1], bo + 1, peers[0], peers[0], 0, z, 0),
                                        (M.PRE_ACCEPT_OK, at, inst[0], inst[1], bo, at, peers[0], 0, z, 0),
                                        (M.ACCEPT_OK, at, inst[0], inst[1], bo, at, peers[0], 0, z, 0)]))
            tid = new_triple()
            w = [rng.randrange(3) for _ in range(n)]
            w[inst[0]] = min(w[inst[0]], inst[1])
            end = 0

            def ok(q, s, vote=(-1, -1), t=-1, ww=None, e=0, b=ballot, seq=0):
                return (at, inst[0], inst[1], b[0], b[1], q, s, vote[0], vote[1], t, seq, list(ww or [0] * n), e)

            dflt, resp = (0, inst[0]), peers[:f]
            if pattern == "noop":
                msgs = [ok(q, R.NOT_SEEN) for q in resp]
            elif pattern == "pre":
                msgs = [ok(q, R.NOT_SEEN) for q in resp[:-1]] + [ok(resp[-1], R.PRE_ACCEPTED, dflt, tid, w, end)]
            elif pattern == "pre_high":
                msgs = [ok(q, R.NOT_SEEN) for q in resp[:-1]] + [ok(resp[-1], R.PRE_ACCEPTED, (1, resp[-1]), tid, w, end)]
            elif pattern == "popular":
                msgs = [ok(q, R.PRE_ACCEPTED, dflt, tid, w, end, seq=2) for q in resp]
            elif pattern == "unpopular":
                msgs = []
                for k, q in enumerate(resp):
                    w2 = list(w)
                    w2[(inst[0] + 1) % n] += k
                    msgs.append(ok(q, R.PRE_ACCEPTED, dflt, tid, w2, end))
            elif pattern == "accepted":
                msgs = [ok(q, R.PRE_ACCEPTED, dflt, tid, w, end) for q in resp[:-1]]
                msgs.append(ok(resp[-1], R.ACCEPTED, (1, resp[-1]), tid + 500, w, end, seq=1))
                commands[tid + 500] = commands[tid]
            else:  # own_column: agreement that holds only because a cover of x and of x + 1 are one set on the own column
                msgs = []
                for k, q in enumerate(resp):
                    w2 = list(w)
                    w2[inst[0]] = inst[1] + (k % 2)
                    msgs.append(ok(q, R.PRE_ACCEPTED, dflt, tid, w2, 0))
            first = msgs[0]
            if event == "stale":
                msgs.insert(0, ok(first[5], R.PRE_ACCEPTED, dflt, tid, w, end, b=(bo - 1, at)))
            elif event == "above":
                msgs.insert(0, ok(first[5], R.NOT_SEEN, b=(bo + 1, at)))
            elif event == "duplicate":
                msgs.insert(0, ok(at, R.NOT_SEEN, (-1, -1), -1))
                msgs.insert(0, ok(at, R.NOT_SEEN, (-1, -1), -1))
            elif event == "replaced":
                msgs.insert(0, ok(first[5] if f > 1 else at, R.ACCEPTED, (2, at), tid + 700, w, end))
                commands[tid + 700] = commands[tid]
                if f == 1:
                    msgs.insert(1, ok(at, R.NOT_SEEN))
            elif event == "own":
                msgs.insert(0, ok(at, R.PRE_ACCEPTED, dflt, tid, w, end))
            elif event == "late":
                msgs.append(ok(peers[-1], R.NOT_SEEN))
            per_instance.append(msgs)
        rng.shuffle(mid)
        for op in mid:
            play(op)
        burst, cursors = [], [0] * len(per_instance)
        live = [k for k, msgs in enumerate(per_instance) if msgs]
        while live:                                                    # interleaved, each instance's own order kept
            k = rng.choice(live)
            burst.append(per_instance[k][cursors[k]])
            cursors[k] += 1
            if cursors[k] == len(per_instance[k]):
                live.remove(k)
        st, rows, decided = play(("prepare_oks", burst, as_intended))
        # ---- the decisions applied: fpx_epx_lead (avoidFastPath) / fpx_epx_lead_accept, then the replies that commit them
        leads, accepts = [], []
        for i in decided:
            (outcome, src, tid, ballot, seq, w, end) = rows[i]
            to, L, x = burst[i][:3]
            if outcome == R.RC_ACCEPT:
                key, is_set = commands[tid]
                accepts.append((L, x, to, ballot >> 3, key, is_set, tid, seq, w, end))
            else:
                tid = NOOP_TRIPLE if outcome == R.RC_PRE_ACCEPT_NOOP else tid
                key, is_set = commands[tid]
                leads.append((L, x, to, ballot >> 3, key, is_set, tid, 1))
        replies = []
        if leads:
            for msg, (w, end) in zip(leads, play(("lead", leads))[1]):
                L, x, to, bo = msg[:4]
                for q in [r for r in range(n) if r != to][:f]:
                    replies.append((M.PRE_ACCEPT_OK, to, L, x, bo, to, q, 0, w, end))
                for q in [r for r in range(n) if r != to][:f]:
                    replies.append((M.ACCEPT_OK, to, L, x, bo, to, q, 0, [0] * n, 0))
        if accepts:
            play(("lead_accept", accepts))
            for (L, x, to, bo) in [a[:4] for a in accepts[::2]]:       # (every other one stays Accepting)
                for q in [r for r in range(n) if r != to][:f]:
                    replies.append((M.ACCEPT_OK, to, L, x, bo, to, q, 0, [0] * n, 0))
        if replies:
            play(("replies", replies))
    return ops, S.census


def random_burst(seed, n, m, num_instances=64, cells=6):
    """(ops that recover `cells` instances, a burst of m PrepareOks over them and a few cells never recovered): heavy
    repetition -- a run is many messages long, most after the decision"""
    rng = random.Random(seed)
    S = R.RecoveryModel(n, 4, num_instances)
    insts = [((k * 2 + 1) % n, k) for k in range(cells)]
    ats = [rng.randrange(n) for _ in insts]
    rec = ("recover", [(i[0], i[1], at) for i, at in zip(insts, ats)])
    res = run_op(S, rec)[1]
    burst = []
    for _ in range(m):
        k = rng.randrange(cells + 2)
        if k >= cells:                                                 # a cell nobody recovers
            burst.append((rng.randrange(n), rng.randrange(n), num_instances - 1, 1, 0, 0, 0, -1, -1, -1, 0, [0] * n, 0))
            continue
        inst, at, bo = insts[k], ats[k], res[k][1]
        s = rng.choice((R.NOT_SEEN, R.NOT_SEEN, R.PRE_ACCEPTED, R.ACCEPTED))
        vote = (-1, -1) if s == R.NOT_SEEN else rng.choice(((0, inst[0]), (1, rng.randrange(n))))
        w = [rng.randrange(2) for _ in range(n)]
        w[inst[0]] = min(w[inst[0]], inst[1])
        b = bo - 1 if rng.random() < 0.1 else bo
        burst.append((at, inst[0], inst[1], b, at, rng.randrange(n), s, vote[0], vote[1], 2000 + rng.randrange(2), 0, w, 0))
    return rec, burst


# ---- runners ---------------------------------------------------------------------------------------------------------------
def run_op(model, op):
    n = model.n
    if op[0] == "recover":
        st, out = model.recover(op[1])
        return (st, None if out is None else [tuple(r) for r in out])
    if op[0] == "prepare_oks":
        st, out, decided = model.prepare_oks(op[1], op[2])
        if st == R.EINVAL:
            return (st, None, None)
        rows = []
        for msg, (outcome, src, tid, ballot, seq, d) in zip(op[1], out):
            w, end = enc_deps(n, (msg[1], msg[2]), d) if outcome == R.RC_ACCEPT else ([0] * n, 0)
            rows.append((outcome, src, tid, ballot, seq, w, end))
        return (st, rows, decided)
    if op[0] == "lead_accept":
        return (model.lead_accept(op[1]),)
    if op[0] == "replies":                                             # (a decided triple known by id alone: -1 in every column)
        st, out, decided = model.replies(op[1])
        if st == M.EINVAL:
            return (st, None, None)
        rows = []
        for i, (msg, (outcome, seq, d, tid)) in enumerate(zip(op[1], out)):
            w, end = enc_deps(n, (msg[2], msg[3]), d) if i in decided else ([0] * n, 0)
            rows.append((outcome, seq, w, end, tid))
        return (st, rows, decided)
    return LS.run_op(model, op)


def prepare_ok_arrays(n, msgs):
    """the input arrays of fpx_epx_recovery_replies for a list of message tuples"""
    cols = list(zip(*[m[:11] for m in msgs])) if msgs else [[]] * 11
    a = [np.asarray(c, np.int32) for c in cols]
    deps = np.asarray([m[11] for m in msgs], np.int32).reshape(len(msgs), n)
    dend = np.asarray([m[12] for m in msgs], np.int32)
    return a + [deps, dend]


def gpu_rows(n, res):
    st, outcome, src, otr, ob, oseq, odeps, oend, dec = res
    if st == R.EINVAL:
        return (st, None, None)
    rows = [(int(outcome[i]), int(src[i]), int(otr[i]), int(ob[i]), int(oseq[i]), [int(v) for v in odeps[i]], int(oend[i]))
            for i in range(len(outcome))]
    return (st, rows, [int(v) for v in dec])


def run_gpu_op(epx, op):
    n = epx.n
    if op[0] == "recover":
        cols = [np.asarray(c, np.int32) for c in zip(*op[1])]
        st, outcome, ord_, os_, ov, ot = epx.recover(*cols)
        if st == R.EINVAL:
            return (st, None)
        return (st, [(int(outcome[i]), int(ord_[i]), int(os_[i]), int(ov[i]), int(ot[i])) for i in range(len(op[1]))])
    if op[0] == "prepare_oks":
        a = prepare_ok_arrays(n, op[1])
        return gpu_rows(n, epx.recovery_replies(*a[:10], a[10], a[11], a[12], as_intended=op[2]))
    if op[0] == "lead_accept":
        cols = list(zip(*[m[:8] for m in op[1]]))
        a = [np.asarray(c, np.int32) for c in cols]
        deps = np.asarray([m[8] for m in op[1]], np.int32)
        dend = np.asarray([m[9] for m in op[1]], np.int32)
        return (epx.lead_accept(a[0], a[1], a[2], a[3], a[4], a[5].astype(np.uint8), a[6], a[7], deps, dend),)
    return LS.run_gpu_op(epx, op)


def touched(ops, step=1):
    cells, keys = set(), set()
    plain = []
    for op in ops:
        if op[0] == "recover":
            cells.update((m[2], (m[0], m[1])) for m in op[1])
        elif op[0] == "prepare_oks":
            cells.update((m[0], (m[1], m[2])) for m in op[1])
        elif op[0] == "lead_accept":
            cells.update((m[2], (m[0], m[1])) for m in op[1])
            keys.update(m[4] for m in op[1])
        else:
            plain.append(op)
    c2, k2 = LS.touched(plain)
    return sorted(cells | set(c2))[::step], sorted(k for k in keys | set(k2) if k >= 0)


def model_state(model, ops, step=1):
    """what the GPU readbacks show, from a RecoveryModel (the form of epaxos_leader_streams.model_state, plus Preparing:
    (3, ballot, {q: (status, vote ballot, triple id, seq, watermarks.., values_end)})"""
    n = model.n
    cells, keys = touched(ops, step)
    out = {}
    for (r, inst) in cells:
        e = model.replicas[r].cmd_log.get(inst)
        if e is None:
            entry, deps = (0, -1, -1, -1), None
        else:
            entry = (e.kind, R.enc(e.ballot), R.enc(e.vote_ballot), e.triple_id)
            deps = None if e.deps is None else LS.encode_deps(n, inst, e.deps)
        st = model.leader_states[r].get(inst)
        if st is None:
            ls = (0,)
        elif isinstance(st, M.PreAccepting):
            resp = {q: (s,) + tuple(LS._flat(LS.encode_deps(n, inst, d))) for q, (s, d) in st.responses.items()}
            ls = (1, R.enc(st.ballot), int(st.avoid_fast_path), st.triple_id, st.key, int(st.is_set), resp)
        elif isinstance(st, M.Accepting):
            s, d = st.triple
            ls = (2, R.enc(st.ballot), st.triple_id, st.key, int(st.is_set), sorted(st.responses),
                  (s,) + tuple(LS._flat(enc_deps(n, inst, d))))
        else:
            ls = (3, R.enc(st.ballot), {q: (p.status, R.enc(p.vote_ballot), p.triple_id, p.seq) +
                                        tuple(LS._flat(enc_deps(n, inst, p.deps))) for q, p in st.responses.items()})
        out[(r, inst)] = (entry, deps, ls)
    largest = [R.enc(rep.largest_ballot) for rep in model.replicas]
    index = {(r, k): (list(model.replicas[r].gets[k]), list(model.replicas[r].sets[k])) for r in range(n) for k in keys}
    return out, largest, index


def gpu_state(epx, ops, step=1):
    n = epx.n
    cells, keys = touched(ops, step)
    out = {}
    for (r, inst) in cells:
        kind, ballot, vote, tid, _ = epx.read_cmdlog(r, inst[0], inst[1])
        d, dend = epx.read_cmdlog_deps(r, inst[0], inst[1])
        # (no entry and a NoCommandEntry hold no triple; a triple known by its id alone shows -1)
        deps = None if (kind in (0, 1) or d[0] == -1) else ([int(v) for v in d], dend)
        if kind == 0:
            ballot = vote = tid = -1
        head, resp = epx.read_leader_state(r, inst[0], inst[1])
        phase, lb, avoid, ltid, key, is_set, mask = head[:7]
        if phase == 0:
            ls = (0,)
        elif phase == 1:
            ls = (1, lb, avoid, ltid, key, is_set, {q: tuple(int(v) for v in resp[q]) for q in range(n) if (mask >> q) & 1})
        elif phase == 2:
            ls = (2, lb, ltid, key, is_set, [q for q in range(n) if (mask >> q) & 1], tuple(int(v) for v in resp[r]))
        else:
            rs = epx.read_recovery_state(r, inst[0], inst[1])
            assert all((rs[q, 0] >= 0) == bool((mask >> q) & 1) for q in range(n))
            ls = (3, lb, {q: tuple(int(v) for v in rs[q]) + tuple(int(v) for v in resp[q]) for q in range(n) if (mask >> q) & 1})
        out[(r, inst)] = ((kind, ballot, vote, tid), deps, ls)
    largest = [epx.read_cmdlog(r, 0, 0)[4] for r in range(n)]
    index = {}
    for r in range(n):
        for k in keys:
            g, s = epx.read_index(r, k)
            index[(r, k)] = ([int(v) for v in g], [int(v) for v in s])
    return out, largest, index
