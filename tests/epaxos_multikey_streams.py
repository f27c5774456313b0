"""epaxos_multikey_streams.py -- test infrastructure: whole BATCHES of EPaxos messages with a key list per command.

tests/epaxos_multikey_sets.py (explicit dependency sets, key tuples) answers one message at a time; include/fpx.h defines
a batch as "message i, in array order, to the replicas of target_mask[i]".  The run_* drivers here apply a batch to the
set model message by message and return the replies in the entry points' own output shapes, with every dependency array
replaced by the SET it stands for; decoded() brings the arrays of a device (or C oracle) call into the same shape through
tests.test_epaxos_models.decode, and assert_same() compares the two.  The set model shares nothing of the watermark /
values-end encoding with the code it checks.

A stream is a list of ops (kind, dict of arrays): multikey_stream() rotates through a pre-accept tick, PreAccept batches
(random ballots, and the old leaders' Ballot(0, leader) once more), Accepts sent and re-sent, Prepares, and Commits with
and without dependencies, over instances in every command-log state (tests.test_epaxos._cl_batch).  What an op holds does
not depend on any answer, so the CPU tests can examine from the model alone the very streams the GPU tests replay."""
import numpy as np

from oracle import epaxos_sets as base
from tests.test_epaxos import _cl_batch
from tests.test_epaxos_models import decode, encode_ballot
from tests.workloads import random_tick

FATAL = 9                    # FPX_EFATAL_PROTOCOL
EMPTY = frozenset()
# (n, NI, m, num_keys) of the multi-key streams the GPU tests replay against the set model: multikey_stream(SEED + n, ...)
# with 0 .. 8 keys per command for STEPS[n] steps (the set model and the state comparison after every batch set the
# pace: two rotations at the smallest shape, one at n = 5, one less its last two steps at n = 7).
# tests/test_epaxos_multikey_streams_cpu.py checks what they reach.
MULTIKEY_SHAPES = [(3, 64, 40, 3), (5, 512, 1100, 8), (7, 300, 1500, 12)]
SEED = 4100
STEPS = {3: 16, 5: 8, 7: 6}


def _targets(mask, n):
    return [r for r in range(n) if (int(mask) >> r) & 1]


def _keys(key_lists, i):
    """the model's command: None for a Noop (key_lists[i] is None), else the key tuple -- () for an empty list"""
    return None if key_lists[i] is None else tuple(int(k) for k in key_lists[i])


# ---- the batch drivers: message i, in array order, at the replicas of target[i] -----------------------------------------
def run_handle_preaccept(model, leader, number, b_ord, b_rep, key_lists, is_set, triple, deps_in, deps_in_end, target):
    """-> (0, ok, resend, nack, commit, nack_ballot, deps[m][n], triple[m][n]); deps[i][r] is the set the reply of
    replica r carried, None for a triple known by its id alone, the empty set where r sent neither PreAcceptOk nor Commit"""
    m, n = len(leader), model.n
    bits = {w: [0] * m for w in ("ok", "resend", "nack", "commit")}
    nb, deps, rt = [-1] * m, [[EMPTY] * n for _ in range(m)], [[-1] * n for _ in range(m)]
    for i in range(m):
        L, x = int(leader[i]), int(number[i])
        din = decode(deps_in[i], L, x, 0 if deps_in_end is None else int(deps_in_end[i]))
        tid = -1 if triple is None else int(triple[i])
        got = model.handle_preaccept((L, x), (int(b_ord[i]), int(b_rep[i])), _keys(key_lists, i), bool(is_set[i]), tid, din,
                                     _targets(target[i], n))
        for r, v in got.items():
            if v[0] == "ignore":
                continue
            bits[v[0]][i] |= 1 << r
            if v[0] == "nack":
                nb[i] = max(nb[i], encode_ballot(v[1]))
            else:
                deps[i][r], rt[i][r] = (None if v[1] is None else frozenset(v[1])), v[2]
    return 0, bits["ok"], bits["resend"], bits["nack"], bits["commit"], nb, deps, rt


def run_accept(model, leader, number, b_ord, b_rep, triple, target, key_lists, is_set):
    """-> (0 | 9, ok, nack, commit, nack_ballot, committed); a message whose proposer refuses is skipped (status 9)"""
    m, n = len(leader), model.n
    st, ok, nack, com, nb, done = 0, [0] * m, [0] * m, [0] * m, [-1] * m, [0] * m
    for i in range(m):
        fatal, got, committed = model.accept((int(leader[i]), int(number[i])), (int(b_ord[i]), int(b_rep[i])), int(triple[i]),
                                             _targets(target[i], n), keys=_keys(key_lists, i), is_set=bool(is_set[i]))
        if fatal:
            st = FATAL
            continue
        done[i] = int(committed)
        for r, v in got.items():
            if v[0] == "ok":
                ok[i] |= 1 << r
            elif v[0] == "commit":
                com[i] |= 1 << r
            else:
                nack[i] |= 1 << r
                nb[i] = max(nb[i], encode_ballot(v[1]))
    return st, ok, nack, com, nb, done


def run_prepare(model, leader, number, b_ord, b_rep, target):
    """-> (0, ok, nack, commit, nack_ballot, reply_status[m][n], reply_vote[m][n], reply_triple[m][n])"""
    m, n = len(leader), model.n
    ok, nack, com, nb = [0] * m, [0] * m, [0] * m, [-1] * m
    rs, rv, rt = ([[-1] * n for _ in range(m)] for _ in range(3))
    for i in range(m):
        got = model.prepare((int(leader[i]), int(number[i])), (int(b_ord[i]), int(b_rep[i])), _targets(target[i], n))
        for r, v in got.items():
            if v[0] == "ok":
                ok[i] |= 1 << r
                rs[i][r], rv[i][r], rt[i][r] = v[1], encode_ballot(v[2]), v[3]
            elif v[0] == "commit":
                com[i] |= 1 << r
            else:
                nack[i] |= 1 << r
                nb[i] = max(nb[i], encode_ballot(v[1]))
    return 0, ok, nack, com, nb, rs, rv, rt


def run_handle_commit(model, leader, number, triple, target, key_lists, is_set, deps=None, deps_end=None):
    for i in range(len(leader)):
        L, x = int(leader[i]), int(number[i])
        d = None if deps is None else decode(deps[i], L, x, 0 if deps_end is None else int(deps_end[i]))
        model.handle_commit((L, x), int(triple[i]), d, _targets(target[i], model.n), keys=_keys(key_lists, i),
                            is_set=bool(is_set[i]))
    return 0


def run_tick(model, leader, number, key_lists, is_set, mask, rank, triple):
    """-> (0, fast, deps[m], leader_deps[m]) of a pre-accept tick of fresh instances, dependencies as sets"""
    out = model.tick(leader, number, [tuple(int(k) for k in ks) for ks in key_lists], is_set, mask, rank, triple_id=triple)
    return 0, [int(f) for f, _, _ in out], [frozenset(d) for _, d, _ in out], [frozenset(D) for _, _, D in out]


# ---- ops: one call each, for the set model, the C oracle (one key per command) and the device ---------------------------
def apply_model(model, op, noop_is_none=False):
    """noop_is_none: hand a command without keys to the model as a Noop (None) instead of the empty list ()"""
    kind, a = op
    kl = a.get("keys")
    if kl is not None and noop_is_none:
        kl = [ks if len(ks) else None for ks in kl]
    if kind == "tick":
        return run_tick(model, a["leader"], a["number"], a["keys"], a["is_set"], a["mask"], a["rank"], a["triple"])
    if kind == "hp":
        return run_handle_preaccept(model, a["leader"], a["number"], a["b_ord"], a["b_rep"], kl, a["is_set"], a["triple"],
                                    a["din"], a["dend"], a["tgt"])
    if kind == "accept":
        return run_accept(model, a["leader"], a["number"], a["b_ord"], a["b_rep"], a["triple"], a["tgt"], kl, a["is_set"])
    if kind == "prepare":
        return run_prepare(model, a["leader"], a["number"], a["b_ord"], a["b_rep"], a["tgt"])
    assert kind == "commit"
    return (run_handle_commit(model, a["leader"], a["number"], a["triple"], a["tgt"], kl, a["is_set"], a["deps"], a["ends"]),)


def apply_single_key(e, op):
    """the single-key entry points (device or C oracle: the same methods) on an op of a one-key stream (a["key"])"""
    kind, a = op
    if kind == "tick":
        return e.preaccept(a["leader"], a["number"], a["key"], a["is_set"], a["mask"], a["rank"], triple_id=a["triple"])
    if kind == "hp":
        return e.handle_preaccept(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["key"], a["is_set"], a["triple"],
                                  a["din"], a["dend"], a["tgt"])
    if kind == "accept":
        return e.accept(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["triple"], a["tgt"], a["key"], a["is_set"])
    if kind == "prepare":
        return e.prepare(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["tgt"])
    assert kind == "commit"
    return (e.handle_commit(a["leader"], a["number"], a["triple"], a["tgt"], key=a["key"], is_set=a["is_set"],
                            deps=a["deps"], deps_values_end=a["ends"]),)


def apply_multikey(e, op):
    """the _mk entry points of the device on any op (a["keys"]); Prepare has no command and no _mk form"""
    kind, a = op
    if kind == "tick":
        return e.preaccept_mk(a["leader"], a["number"], a["keys"], a["is_set"], a["mask"], a["rank"], triple_id=a["triple"])
    if kind == "hp":
        return e.handle_preaccept_mk(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["keys"], a["is_set"], a["triple"],
                                     a["din"], a["dend"], a["tgt"])
    if kind == "accept":
        return e.accept_mk(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["triple"], a["tgt"], a["keys"], a["is_set"])
    if kind == "prepare":
        return e.prepare(a["leader"], a["number"], a["b_ord"], a["b_rep"], a["tgt"])
    assert kind == "commit"
    return (e.handle_commit_mk(a["leader"], a["number"], a["triple"], a["tgt"], a["keys"], a["is_set"], deps=a["deps"],
                               deps_values_end=a["ends"]),)


def _reply_sets(leader, number, rd, re):
    out = []
    for i in range(len(leader)):
        L, x = int(leader[i]), int(number[i])
        row = []
        for r in range(rd.shape[1]):
            if rd[i, r, 0] == -1:
                row.append(None)
            elif not re[i, r] and not rd[i, r].any():
                row.append(EMPTY)
            else:
                row.append(frozenset(decode(rd[i, r], L, x, int(re[i, r]))))
        out.append(row)
    return out


def decoded(op, out):
    """the arrays an entry point returned for `op`, in the shape of the run_* drivers: dependency arrays as sets"""
    kind, a = op
    out = tuple(out)
    L, x = a["leader"], a["number"]
    if kind == "tick":
        st, fast, deps, ldeps, own = out
        return (int(st), fast.tolist(), [frozenset(decode(deps[i], int(L[i]), int(x[i]), int(own[i][0]))) for i in range(len(L))],
                [frozenset(decode(ldeps[i], int(L[i]), int(x[i]), int(own[i][1]))) for i in range(len(L))])
    if kind == "hp":
        st, ok, resend, nack, com, nb, rd, re, rt = out
        return (int(st), ok.tolist(), resend.tolist(), nack.tolist(), com.tolist(), nb.tolist(), _reply_sets(L, x, rd, re),
                rt.tolist())
    return tuple(v.tolist() if isinstance(v, np.ndarray) else int(v) for v in out)


FIELDS = {"tick": ("status", "fast", "deps", "leader_deps"),
          "hp": ("status", "ok", "resend", "nack", "commit", "nack_ballot", "reply_deps", "reply_triple"),
          "accept": ("status", "ok", "nack", "commit", "nack_ballot", "committed"),
          "prepare": ("status", "ok", "nack", "commit", "nack_ballot", "reply_status", "reply_vote", "reply_triple"),
          "commit": ("status",)}


def _shown(g, w):
    if isinstance(g, frozenset) and isinstance(w, frozenset):
        return "%d instances too many %r, %d missing %r" % (len(g - w), sorted(g - w)[:6], len(w - g), sorted(w - g)[:6])
    return ("%r != %r" % (g, w))[:400]


def first_difference(kind, got, want):
    """'' when the two results are the same, else the first field and message at which they differ"""
    for name, g, w in zip(FIELDS[kind], got, want):
        if g == w:
            continue
        if not isinstance(g, list):
            return "%s: %r != %r" % (name, g, w)
        i = next(i for i in range(len(w)) if g[i] != w[i])
        if isinstance(g[i], list):
            r = next(r for r in range(len(w[i])) if g[i][r] != w[i][r])
            return "%s[%d][%d]: %s" % (name, i, r, _shown(g[i][r], w[i][r]))
        return "%s[%d]: %s" % (name, i, _shown(g[i], w[i]))
    return ""


def assert_same(op, got, want):
    """every reply of every message of the batch: `got` (decoded()) against the set model's `want`"""
    assert len(got) == len(want) == len(FIELDS[op[0]])
    assert got == want, "%s batch of %d: %s" % (op[0], len(op[1]["leader"]), first_difference(op[0], got, want))


def compare_state(gpu, model, n, NI, num_keys, instances):
    """the command log (kind, ballot, vote ballot, triple id, largestBallot, the stored dependencies as a set) of the
    given (leader, number) instances at every replica, and every key's gets / sets rows at every replica"""
    for r in range(n):
        rep = model.replicas[r]
        largest = encode_ballot(rep.largest_ballot)
        for L, x in instances:
            assert 0 <= x < NI
            kind, ballot, vote, tid, lb = gpu.read_cmdlog(r, L, x)
            assert lb == largest, (r, L, x, lb, largest)
            e = rep.cmd_log.get((L, x))
            if e is None:
                assert kind == base.NONE, (r, L, x, kind)
                continue
            assert (kind, ballot, vote, tid) == (e.kind, encode_ballot(e.ballot), encode_ballot(e.vote_ballot), e.triple_id), (r, L, x)
            if e.kind in (base.PRE_ACCEPTED, base.ACCEPTED, base.COMMITTED):
                wm, end = gpu.read_cmdlog_deps(r, L, x)
                if e.deps is None:
                    assert wm[0] == -1, (r, L, x, wm)
                else:
                    assert wm[0] != -1 and decode(wm, L, x, end) == set(e.deps), (r, L, x)
        for k in range(num_keys):
            g, s = gpu.read_index(r, k)
            assert g.tolist() == rep.gets[k] and s.tolist() == rep.sets[k], (r, k)


# ---- stream generators -----------------------------------------------------------------------------------------------
def random_key_lists(rng, m, num_keys, max_keys):
    """0 .. max_keys keys per command with repeats; one command in twelve is one key several times over"""
    lists = [rng.integers(0, num_keys, int(c)).tolist() for c in rng.integers(0, max_keys + 1, m)]
    for i in np.nonzero(rng.random(m) < 1 / 12)[0]:
        lists[i] = [int(rng.integers(0, num_keys))] * int(rng.integers(2, max(3, max_keys + 1)))
    return lists


def lists_of(key):
    """one-key commands as key lists: [k], and the empty list for a Noop (key -1)"""
    return [[int(k)] if k >= 0 else [] for k in key]


def _commands(rng, mm, num_keys, max_keys, noops=True):
    """-> (key or None, key lists): max_keys None = the one-key stream, a key (or -1, a Noop) per command"""
    if max_keys is None:
        key = rng.integers(-1 if noops else 0, num_keys, mm).astype(np.int32)
        return key, lists_of(key)
    return None, random_key_lists(rng, mm, num_keys, max_keys)


def _deps(rng, NI, n, leader, number):
    """dependencies as a message carries them: n watermarks; the own-leader column is a plain watermark <= the instance
    number, or (3 in 10) the number itself with explicit ids above it, up to values_end"""
    mm = len(leader)
    d = rng.integers(0, NI, (mm, n)).astype(np.int32)
    ar = np.arange(mm)
    hole = rng.random(mm) < 0.3
    d[ar, leader] = np.where(hole, number, np.minimum(d[ar, leader], number))
    end = np.where(hole, number + 2 + rng.integers(0, 5, mm), 0).astype(np.int32)
    return d, end


CYCLE = ("tick", "hp", "accept", "hp_old", "prepare", "commit", "hp", "commit_by_id")


def multikey_stream(seed, n, NI, m, num_keys, max_keys=8, steps=len(CYCLE)):
    """the ops of `steps` steps of CYCLE (an Accept step is the batch and the same batch again); max_keys None: the
    one-key stream (every op also carries "key", -1 = Noop, for the single-key entry points)"""
    rng = np.random.default_rng(seed)
    nxt = [0] * n
    ops = []
    for step in range(steps):
        kind = CYCLE[step % len(CYCLE)]
        mm = min(m, 200)
        if kind == "tick" and max(nxt) + mm // 2 + 8 < NI // 2:
            leader, number, key, is_set, mask, rank = random_tick(rng, n, num_keys, mm, nxt, 3.0, fifo=bool(step & 8))
            keys = lists_of(key) if max_keys is None else random_key_lists(rng, mm, num_keys, max_keys)
            triple = rng.integers(0, 1 << 20, mm).astype(np.int32)
            ops.append(("tick", dict(leader=leader, number=number, key=key, keys=keys, is_set=is_set, mask=mask, rank=rank,
                                     triple=triple)))
            continue
        leader, number, b_ord, b_rep, tgt = _cl_batch(rng, n, NI, m, nxt)
        mm = len(leader)
        a = dict(leader=leader, number=number, b_ord=b_ord, b_rep=b_rep, tgt=tgt)
        if kind == "prepare":
            ops.append(("prepare", a))
            continue
        a["key"], a["keys"] = _commands(rng, mm, num_keys, max_keys)
        a["is_set"] = (rng.random(mm) < 0.5).astype(np.uint8)
        a["triple"] = rng.integers(0, 1 << 20, mm).astype(np.int32)
        if kind == "accept":
            a["tgt"] = (tgt & ~(1 << b_rep)).astype(np.uint8)          # an Accept never targets its proposer
            ops += [("accept", a), ("accept", a)]
        elif kind in ("commit", "commit_by_id"):
            a["deps"], a["ends"] = _deps(rng, NI, n, leader, number) if kind == "commit" else (None, None)
            ops.append(("commit", a))
        else:
            a["din"], a["dend"] = _deps(rng, NI, n, leader, number)
            if kind == "hp_old":                                       # the old leaders' original PreAccepts once more
                b_ord[:], b_rep[:] = 0, leader
            ops.append(("hp", a))
    return ops


def hp_op(rng, n, NI, m, num_keys, nxt, keys=None, max_keys=8):
    """one PreAccept batch over _cl_batch's instances; keys: the batch's key lists, else random ones"""
    leader, number, b_ord, b_rep, tgt = _cl_batch(rng, n, NI, m, nxt)
    mm = len(leader)
    din, dend = _deps(rng, NI, n, leader, number)
    return ("hp", dict(leader=leader, number=number, b_ord=b_ord, b_rep=b_rep, tgt=tgt, din=din, dend=dend,
                       keys=random_key_lists(rng, mm, num_keys, max_keys) if keys is None else keys(mm),
                       is_set=(rng.random(mm) < 0.5).astype(np.uint8), triple=rng.integers(0, 1 << 20, mm).astype(np.int32)))


def tick_op(rng, n, m, num_keys, nxt, max_keys=8):
    leader, number, _, is_set, mask, rank = random_tick(rng, n, num_keys, m, nxt, 3.0)
    return ("tick", dict(leader=leader, number=number, keys=random_key_lists(rng, m, num_keys, max_keys), is_set=is_set,
                         mask=mask, rank=rank, triple=rng.integers(0, 1 << 20, m).astype(np.int32)))


def instances_of(op):
    return [(int(L), int(x)) for L, x in zip(op[1]["leader"], op[1]["number"])]


def sampled_instances(rng, n, NI, count):
    return [(int(i) // NI, int(i) % NI) for i in rng.choice(n * NI, size=min(count, n * NI), replace=False)]


# ---- what a stream reaches, from the model's answers alone ------------------------------------------------------------
def popcount(xs):
    return sum(bin(int(v)).count("1") for v in xs)


def coverage(n, ops, results):
    """counts over the stream's replies, and the shape facts of its PreAccept batches"""
    c = dict(ok=0, resend=0, nack=0, commit=0, ignored=0, fatal=0, committed=0, zero_keys=0, repeated_key=0, one_distinct=0,
             split_pair=0, big_batch=0, big_batch_late_nack=0)
    for (kind, a), res in zip(ops, results):
        for ks in a.get("keys") or ():
            c["zero_keys"] += len(ks) == 0
            c["repeated_key"] += len(set(ks)) < len(ks)
            c["one_distinct"] += len(ks) > 1 and len(set(ks)) == 1
        if kind == "accept":
            c["fatal"] += res[0] == FATAL
            c["committed"] += sum(res[5])
            c["nack"] += popcount(res[2])
        elif kind == "hp":
            st, ok, resend, nack, com = res[:5]
            for name, bits in (("ok", ok), ("resend", resend), ("nack", nack), ("commit", com)):
                c[name] += popcount(bits)
            c["ignored"] += popcount(int(t) & ~(o | r | k | q) for t, o, r, k, q in zip(a["tgt"], ok, resend, nack, com))
            c["split_pair"] += split_pair(a["keys"], ok)
            m, P = len(ok), sum(len(ks) for ks in a["keys"])
            if m > 1024 and P > 4096 and P % 4:
                c["big_batch"] += 1
                c["big_batch_late_nack"] += any(nack[1024:])
    return c


def split_pair(key_lists, ok):
    """1 if two messages of the batch share a key, both were processed at one replica and only one of them at another"""
    by_key = {}
    for i, ks in enumerate(key_lists):
        for k in set(ks):
            by_key.setdefault(k, []).append(i)
    for idx in by_key.values():
        bits = np.array([ok[i] for i in idx[:400]], np.int64)
        both, one = bits[:, None] & bits[None, :], bits[:, None] ^ bits[None, :]
        if ((both != 0) & (one != 0)).any():
            return 1
    return 0
