"""Deterministic EPaxos pre-accept ticks that sit exactly at the limits of the tick's kernels (K5: fpx_epaxos.hip,
fpx_epaxos_kp.hpp), built from explicit rank rows.  tests/test_epaxos_tick_shapes_cpu.py checks every tick here against
the oracle and against what its name claims, without a GPU; tests/test_gpu_epaxos_tick_paths.py runs them on the GPU and
proves through fpx_epx_tick_census (include/fpx.h) which path each one took.

A tick is the tuple (leader, number, key, is_set, resp_mask, rank, seen_mask) that EPaxos.preaccept takes.  Instance
numbers follow workloads.random_tick's rule: a leader numbers its instances in the order IT processes them.

LIMITS restates the kernels' exact-fit constants only so that ticks can be built without a GPU; the GPU tests compare it
with what fpx_epx_limits reports.  bucket_of restates the bucket sort's `(rank - lo) >> sh` for the same purpose: it
places commands, the census is the proof that the kernel saw them there."""
import numpy as np

LIMITS = {
    3: dict(kp_tc=1536, key_tc=2048, nbk=1024, kp_max_occ=24, kp_maxb=2048, kp_waves=4),
    5: dict(kp_tc=1152, key_tc=1152, nbk=1024, kp_max_occ=24, kp_maxb=2048, kp_waves=3),
    7: dict(kp_tc=640, key_tc=576, nbk=512, kp_max_occ=24, kp_maxb=2048, kp_waves=2),
}


# ------------------------------------------------------------------------------------------------------ rank rows
def rank_rows(kind, n, m, seed=0):
    """[n][m] rank rows.  identity: every replica processes the tick in message order.  reversed: the last replica in
    exactly the opposite order (its channels reorder: what random_tick's fifo=False allows).  uniform: an independent
    uniform permutation per replica"""
    rank = np.tile(np.arange(m, dtype=np.int32), (n, 1))
    if kind == "reversed":
        rank[n - 1] = rank[n - 1, ::-1]
    elif kind == "uniform":
        rng = np.random.default_rng(seed)
        for r in range(n):
            rank[r] = rng.permutation(m).astype(np.int32)
    else:
        assert kind == "identity", kind
    return rank


def assemble(n, key, rank, leader=None, avoid=None, everybody=False, next_number=None):
    """the tick of commands on `key` with rank rows `rank`.  leader: per command (default i % n).  The one non-leader whose
    answer is not waited for is avoid[i] where that is given (>= 0) and is not the leader, else it rotates with i.
    everybody: seen_mask = all other replicas (the reference's NotThrifty), else the thrifty seen_mask = resp_mask.
    next_number: [n] the leaders' next instance numbers, advanced in place (None: from 0)"""
    key = np.ascontiguousarray(key, np.int32)
    m = len(key)
    i = np.arange(m)
    leader = (i % n).astype(np.int32) if leader is None else np.ascontiguousarray(leader, np.int32)
    others = np.array([[r for r in range(n) if r != L] for L in range(n)])      # [n][n - 1]
    drop = others[leader, (i // n) % (n - 1)]
    if avoid is not None:
        avoid = np.asarray(avoid)
        drop = np.where((avoid >= 0) & (avoid != leader), avoid, drop)
    full = (1 << n) - 1
    resp = (full & ~(1 << leader) & ~(1 << drop)).astype(np.uint8)
    seen = (full & ~(1 << leader)).astype(np.uint8) if everybody else resp.copy()
    is_set = ((i * 7 + key) % 3 != 0).astype(np.uint8)
    number = np.zeros(m, np.int32)
    nxt = [0] * n if next_number is None else next_number
    for L in range(n):
        idx = np.nonzero(leader == L)[0]
        by_own = idx[np.argsort(rank[L, idx], kind="stable")]
        number[by_own] = nxt[L] + np.arange(len(idx))
        nxt[L] += len(idx)
    return leader, number, key, is_set, resp, np.ascontiguousarray(rank, np.int32), seen


def args(tick):
    """(leader, number, key, is_set, resp_mask, rank) and the seen_mask keyword of EPaxos.preaccept"""
    return tick[:6], dict(seen_mask=tick[6])


# ------------------------------------------------------------------------------------------- what a tick looks like
def shift_of(span1, nbk):
    """the bucket sort's shift for ranks lo .. lo + span1 (span1 = span - 1)"""
    return max(0, int(span1 | 1).bit_length() - (nbk.bit_length() - 1))


def bucket_of(rank, lo, span1, nbk):
    return (np.asarray(rank, np.int64) - lo) >> shift_of(span1, nbk)


def participates(tick):
    """[n][m] bool: replica r processes command i (it leads it or is in its seen_mask)"""
    leader, seen = tick[0], tick[6]
    n = tick[5].shape[0]
    part = seen.astype(np.int64) | (1 << leader.astype(np.int64))
    return np.array([(part >> r) & 1 for r in range(n)], bool)


def key_sizes(tick, num_keys):
    return np.bincount(tick[2], minlength=num_keys)


def occupancy(tick, k, attempt=1):
    """the fullest rank bucket of key k over the replicas, as (words, replica, bucket), in the bucket sort's first attempt
    (buckets over the tick's ranks) or its second (over the key's own ranks at that replica); (0, -1, -1) for a key no
    replica has a word of"""
    n, m = tick[5].shape
    nbk = LIMITS[n]["nbk"]
    mine = tick[2] == k
    part = participates(tick)
    best = (0, -1, -1)
    for r in range(n):
        rk = tick[5][r, mine & part[r]]
        if len(rk) == 0:
            continue
        lo, span1 = (0, max(m - 1, 0)) if attempt == 1 else (int(rk.min()), int(rk.max() - rk.min()))
        counts = np.bincount(bucket_of(rk, lo, span1, nbk), minlength=nbk)
        assert len(counts) == nbk, "a rank outside the bucket table"
        q = int(counts.argmax())
        if counts[q] > best[0]:
            best = (int(counts[q]), r, q)
    return best


def route(tick, k):
    """the sort route the restated bucket function predicts for key k: "bucket1", "bucket2", "radix<passes>" or None for an
    empty key.  For the CPU checks of the builders only"""
    n, m = tick[5].shape
    if not (tick[2] == k).any():
        return None
    occ = LIMITS[n]["kp_max_occ"]
    if occupancy(tick, k, 1)[0] <= occ:
        return "bucket1"
    if occupancy(tick, k, 2)[0] <= occ:
        return "bucket2"
    return "radix%d" % ((int(m).bit_length() + 6) // 7)


def routes(tick, num_keys):
    out = {}
    for k in range(num_keys):
        r = route(tick, k)
        if r:
            out[r] = out.get(r, 0) + 1
    return out


# ------------------------------------------------------------------------------------------------------- the ticks
def placed(n, m, groups, fill_keys, lead=None, avoid=None, everybody=False, kind="identity", next_number=None):
    """m commands: key k's are the message indices groups[k]; every other message goes to the keys fill_keys in turn (so
    that with identity ranks a bucket of 32 ranks holds 32 / len(fill_keys) of each).  lead / avoid: {key: replica} -- who
    leads all of that key's commands / whose answer none of them waits for"""
    key = np.asarray(fill_keys, np.int32)[np.arange(m) % len(fill_keys)]
    for k, idx in groups.items():
        key[np.asarray(idx, np.int64)] = k
    leader = (np.arange(m) % n).astype(np.int32)
    av = np.full(m, -1, np.int64)
    for k, L in (lead or {}).items():
        leader[key == k] = L
    for k, r in (avoid or {}).items():
        av[key == k] = r
    return assemble(n, key, rank_rows(kind, n, m), leader=leader, avoid=av, everybody=everybody, next_number=next_number)


def bucket_width(n, m):
    return 1 << shift_of(m - 1, LIMITS[n]["nbk"])


def one_bucket(n, m, members, bucket=3, num_keys=40, extra=None):
    """identity ranks; key 0 has `members` commands, all led by replica 0 (which therefore has a word of each), in rank
    bucket `bucket` of the first attempt, and nothing else unless extra = more message indices; keys 1 .. num_keys - 1 share
    the other messages evenly (40 keys: no key of a tick of 20000 outgrows the on-chip tables, whatever n)"""
    w = bucket_width(n, m)
    assert members <= w, "a bucket of %d ranks cannot hold %d" % (w, members)
    idx = list(range(bucket * w, bucket * w + members)) + list(extra or [])
    return placed(n, m, {0: idx}, list(range(1, num_keys)), lead={0: 0})


def clumps(n, m, size=150, num_keys=40):
    """identity ranks; key 0 = the first `size` and the last `size` messages, led by replica 0: its buckets at both ends of
    the tick overflow, and so do the same buckets over its own rank range, which is the whole tick"""
    idx = list(range(size)) + list(range(m - size, m))
    return placed(n, m, {0: idx}, list(range(1, num_keys)), lead={0: 0})


def many_small_buckets(n, m, members, groups=40, num_keys=80):
    """keys 0 .. groups - 1 each hold `members` neighbouring messages at the start of a bucket of their own, all led by the
    last replica, whose ranks are REVERSED: a key's words reach their bucket in slot order, which is message order, so with
    ascending ranks the bucket's last member would be its largest word -- the one no other member has to count.  Reversed, the
    member read last is the smallest.  The other keys share the rest"""
    w = bucket_width(n, m)
    assert members <= w and m % w == 0, "the reversed ranks of a group's messages lie in one bucket as well"
    g = {k: list(range((3 + 5 * k) * w, (3 + 5 * k) * w + members)) for k in range(groups)}
    assert (3 + 5 * groups) * w <= m
    return placed(n, m, g, list(range(groups, num_keys)), lead={k: n - 1 for k in range(groups)}, kind="reversed")


def last_bucket(n, members=6, num_keys=40):
    """m = 16384 identity ranks: the tick's last rank lies in bucket NBK - 1, and key 0 owns the last `members` ranks"""
    m = 16384
    assert int(bucket_of(m - 1, 0, m - 1, LIMITS[n]["nbk"])) == LIMITS[n]["nbk"] - 1
    return placed(n, m, {0: list(range(m - members, m))}, list(range(1, num_keys)), lead={0: 0})


def last_bucket_second_attempt(n, m=20000, num_keys=40):
    """identity ranks; key 0 = 30 neighbours at the start of one first-attempt bucket (more than it takes) and the two
    ranks 2 NBK - 2, 2 NBK - 1 above the first of them: over the key's own range of 2 NBK ranks a bucket is two ranks wide
    and the last two share bucket NBK - 1"""
    w, nbk = bucket_width(n, m), LIMITS[n]["nbk"]
    assert w >= 30
    at = 5 * w
    idx = list(range(at, at + 30)) + [at + 2 * nbk - 2, at + 2 * nbk - 1]
    return placed(n, m, {0: idx}, list(range(1, num_keys)), lead={0: 0})


def sizes(n, counts, seed=0, everybody=False, kind="identity", next_number=None, lead0=False):
    """key k has counts[k] commands, spread over the tick by a seeded shuffle"""
    key = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    key = key[np.random.default_rng(seed).permutation(len(key))]
    m = len(key)
    rank = rank_rows(kind, n, m, seed)
    leader = np.zeros(m, np.int32) if lead0 else None
    return assemble(n, key, rank, leader=leader, everybody=everybody, next_number=next_number)


def key_size_counts(n):
    """0, 1, 63, 64, 65 commands, either side of W * 64 (one 64-command chunk per wavefront), TC - 1 and TC"""
    L = LIMITS[n]
    w64 = L["kp_waves"] * 64
    return [0, 1, 63, 64, 65, w64 - 1, w64, w64 + 1, L["kp_tc"] - 1, L["kp_tc"]]


def absent_replica(n, m=3000, num_keys=6, everybody=False):
    """replica n - 1 leads no command of key 0 and none of them waits for its answer (n = 3: every command of key 0 is led
    by replica 0 or 1 with the other as the sole responder); with the thrifty masks it takes part in none of them"""
    key = (np.arange(m) % num_keys).astype(np.int32)
    leader = (np.arange(m) % n).astype(np.int32)
    k0 = key == 0
    leader[k0] = (np.arange(m)[k0] // num_keys) % (n - 1)
    avoid = np.where(k0, n - 1, -1)
    return assemble(n, key, rank_rows("identity", n, m), leader=leader, avoid=avoid, everybody=everybody)


def bit20(n=5, num_keys=2048):
    """2^20 + 2052 commands, key = i % 2048: ranks and indices above 2^20.  Replica 2 processes the tick leader by leader
    (all of leader 0's commands, then leader 1's, ...), the last replica -- whose rank is the one the record splits into two
    halves -- leader by leader from the last leader down, the others in message order: every channel stays FIFO (the
    oracle keeps the explicit values of a reordered channel as sets, a million of them do not fit a test), and no command
    but the first few keeps its rank.  A rank bucket is 2048 ranks wide: it holds two commands of a key at most, whichever
    replica"""
    m = (1 << 20) + 2052
    i = np.arange(m)
    rank = rank_rows("identity", n, m)
    rank[2, np.lexsort((i, i % n))] = i
    rank[n - 1, np.lexsort((i, n - 1 - i % n))] = i
    key = (i % num_keys).astype(np.int32)
    return assemble(n, key, rank)
