"""Seeded synthetic command streams of SURVEY.md section 8(d), as backend-agnostic op scripts.

A script is a list of ops; `run_script(backend, script)` applies it to either the oracle
(`oracle.pyoracle.System`) or the GPU (`frankenpaxos_amd.Context`) -- both expose the same methods --
and returns every output, so parity is `assert_same(run_script(gpu), run_script(oracle))`.
"""
import numpy as np

MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64_at(x):
    """one splitmix64 output for each state in x (vectorised, wrap-around uint64 arithmetic)"""
    with np.errstate(over="ignore"):
        z = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def steady_values(slots):
    """value_id[i] = splitmix64(seed = 0xF9A405 + i) & 0x7fffffff   (steady stream)"""
    return (splitmix64_at(np.asarray(slots, dtype=np.uint64) + np.uint64(0xF9A405))
            & np.uint64(0x7FFFFFFF)).astype(np.int32)


def steady_stream(S, start=0):
    slot = np.arange(start, start + S, dtype=np.int32)
    return slot, np.zeros(S, np.int32), steady_values(slot)


class Rng:
    def __init__(self, seed):
        self.s = np.uint64(seed)

    def next(self):
        with np.errstate(over="ignore"):
            self.s = self.s + np.uint64(0x9E3779B97F4A7C15)
        z = self.s
        with np.errstate(over="ignore"):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))

    def below(self, n):
        return self.next() % n

    def chance(self, num, den):
        return self.below(den) < num

    def np_rng(self):
        return np.random.default_rng(self.next() & 0xFFFFFFFF)


def bits_from_bool(mat):
    """bool [n, total] -> uint64 [n, 4] little-endian bitmaps"""
    n, total = mat.shape
    padded = np.zeros((n, 256), np.uint8)
    padded[:, :total] = mat
    by = np.packbits(padded, axis=1, bitorder="little")  # [n, 32] bytes
    return by.view(np.uint64).reshape(n, 4).copy()


def bool_from_bits(bits, total):
    by = np.ascontiguousarray(bits, dtype=np.uint64).view(np.uint8).reshape(-1, 32)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :total].astype(bool)


def random_subsets(nprng, n, total, lo, hi):
    """n random subsets of [0, total), sizes uniform in [lo, hi]"""
    sizes = nprng.integers(lo, hi + 1, size=n)
    keys = nprng.random((n, total))
    order = np.argsort(keys, axis=1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(total)[None, :].repeat(n, 0), axis=1)
    return rank < sizes[:, None]


def fast_subsets(nprng, n, total, lo, hi):
    """n pseudo-random subsets of [0, total) with sizes uniform in [lo, hi], in O(n * total) byte operations
    (random_subsets sorts n x total keys: minutes at 2^20 x 256).  total must be a power of two <= 256: member j
    of subset i is (a_i * j + b_i) mod total for j < size_i with a_i odd -- j -> a j + b is a permutation of
    Z/total, so the size is exact.  Used by the full-size parity streams; which acceptors a Phase2a reaches is
    the caller's choice in the reference too (an unseeded shuffle)."""
    assert total & (total - 1) == 0 and total <= 256
    sizes = nprng.integers(lo, hi + 1, size=n)
    a = (nprng.integers(0, total // 2 if total > 1 else 1, size=n) * 2 + 1).astype(np.int64)
    b = nprng.integers(0, total, size=n).astype(np.int64)
    # position of element e in subset i's order: j = a^-1 (e - b) mod total ; member iff j < size
    inv = np.array([pow(int(x), -1, total) if total > 1 else 0 for x in range(1, 2 * total, 2)], np.int64)
    ainv = inv[(a - 1) // 2 % len(inv)]
    e = np.arange(total, dtype=np.int64)[None, :]
    j = (ainv[:, None] * (e - b[:, None])) & (total - 1)
    return j < sizes[:, None]


def run_subsets(nprng, n, total, lo, hi):
    """n RUNS of neighbouring acceptors: positions [start, start + len) of the 256 a row has room for, cyclically, start a
    multiple of 16 (a 64-byte sector of the row), len uniform in [lo, min(hi, 128)]; positions >= total have no
    acceptor.  What a thrifty proxy leader sends when it rotates a window of f + 1 acceptors over the group instead of
    shuffling (any f + 1 will do: multipaxos/ProxyLeader.scala:190-191) -- the delivery k_phase2's packed walk takes."""
    start = 16 * nprng.integers(0, 16, size=n)
    length = nprng.integers(lo, min(hi, 128) + 1, size=n)
    j = np.arange(256)[None, :]
    return ((((j - start[:, None]) % 256) < length[:, None]) & (j < total))[:, :total]


def next_classic_round(n, leader, rnd):
    if rnd < 0:
        return leader
    m = n * (rnd // n)
    off = leader % n
    return m + off if m + off > rnd else m + n + off


def adversarial_script(S, R, q, seed, epochs=64, num_leaders=2, fused=True, ngroups=1,
                       group_of=None, subsets=None):
    """The parity / adversarial stream of SURVEY.md 8(d): delivery in `epochs` epochs of S/epochs
    slots; before an epoch, with probability 1/4, a leader change bumps the proposing round to
    nextClassicRound(leader = e % 2, round) and a random 25 % of the acceptors is pre-promised to the
    new round (Phase1a), so stale Phase2a's get Nacked; after a leader change 5 % of the already
    proposed slots are re-proposed in the new round with the same value; target_mask is a random
    subset of size U[q-8, R] (clamped to [1, R]); in the unfused pipeline 10 % of the vote messages
    are delivered twice.  Every epoch is one batch, so a batch carries one round per group."""
    subsets = subsets or random_subsets
    rng = Rng(seed)
    ops = []
    rnd = 0
    per = max(1, S // epochs)
    values = steady_values(np.arange(S))
    proposed = 0
    # the leader of round 0 runs Phase 1 first (all acceptors promise round 0)
    for g in range(ngroups):
        ops.append(("phase1a", g, 0, 0, None))
    e = 0
    pending_round = None
    while proposed < S:
        lo, hi = proposed, min(S, proposed + per)
        reprop = np.zeros(0, np.int64)
        if pending_round is not None:
            # the new leader finishes Phase 1 with everybody and takes over; it re-proposes 5 % of
            # the old slots in its round with the same value (Paxos-safe)
            rnd = pending_round
            pending_round = None
            nprng = rng.np_rng()
            for g in range(ngroups):
                ops.append(("phase1a", g, rnd, 0, None))
            if lo > 0:
                k = max(1, lo // 20)
                reprop = np.sort(nprng.choice(lo, size=k, replace=False))
        elif e > 0 and rng.chance(1, 4):
            # a competing leader pre-promises 25 % of the acceptors to its next round; the current
            # leader keeps proposing in the old round during this epoch => those acceptors Nack
            pending_round = next_classic_round(num_leaders, e % 2, rnd)
            if pending_round == rnd:
                pending_round = next_classic_round(num_leaders, e % 2, rnd + 1)
            nprng = rng.np_rng()
            pre = random_subsets(nprng, 1, R, max(1, R // 4), max(1, R // 4))
            for g in range(ngroups):
                ops.append(("phase1a", g, pending_round, 0, bits_from_bool(pre)[0]))
        nprng = rng.np_rng()
        slot = np.concatenate([reprop, np.arange(lo, hi)]).astype(np.int32)
        rr = np.full(len(slot), rnd, np.int32)
        val = values[slot]
        tgt = bits_from_bool(subsets(nprng, len(slot), R, max(1, q - 8), R))
        if fused:
            ops.append(("fused", slot, rr, val, tgt))
        else:
            dup = nprng.random(len(slot)) < 0.10
            ops.append(("k1k2", slot, rr, val, tgt, dup))
        proposed = hi
        e += 1
    return ops


def shaped(script, delivery, solo_every=2, solo_n=400):
    """a script with its vote batches delivered as a case asks: no target masks when dense; every `solo_every`-th batch cut
    into pieces of at most `solo_n` messages (each a solo launch), the others whole"""
    out, k = [], 0
    for op in script:
        if op[0] not in ("fused", "k1k2"):
            out.append(op)
            continue
        op = list(op)
        if delivery == "dense":
            op[4] = None
        n = len(op[1])
        size = solo_n if solo_every and k % solo_every == 1 else max(n, 1)
        for lo in range(0, n, size):
            out.append(tuple([op[0]] + [None if a is None else a[lo:lo + size] for a in op[1:]]))
        k += 1
    return out


def band_on_device(fa, gpu, fused_op, ranges_op, independent):
    """one proxy-leader step through fpx_mencius_band_fused_dev on device-resident arrays; returns the sync status and the
    two halves' outputs in the order of phase2_fused / noop_ranges_fused"""
    import torch
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _, slot, rr, val, tgt = fused_op
    _, st_, en_, rn_, tm = ranges_op
    n, k, A = len(slot), len(st_), gpu.cfg.num_groups
    ch, cr, cv, nr = (torch.zeros(n, dtype=torch.uint8, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev),
                      torch.full((n,), -1, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev))
    vb, nb = (torch.zeros((k, A, 4), dtype=torch.int64, device=dev) for _ in range(2))
    rnr, new, rch = (torch.full((k,), -1, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.uint8, device=dev),
                     torch.zeros(k, dtype=torch.uint8, device=dev))
    gpu.mencius_band_fused_dev(d(slot), d(rr), d(val), None if tgt is None else d(tgt.view(np.int64)), ch, cr, cv, nr, d(st_), d(en_),
                               d(rn_), d(np.ascontiguousarray(tm).view(np.int64)), vb, nb, rnr, new, rch, independent=independent)
    st = gpu.sync()
    h = lambda t: t.cpu().numpy()
    return st, (h(ch), h(cr), h(cv), h(nr)), (h(vb).view(np.uint64), h(nb).view(np.uint64), h(rnr), h(new), h(rch))


def run_script(be, script):
    """apply a script to a backend; returns a list of (tag, arrays...) outputs"""
    out = []
    for op in script:
        kind = op[0]
        if kind == "phase1a":
            _, g, rnd, wm, tgt = op
            st, pb, nb = be.acceptor_phase1a(g, rnd, wm, tgt)
            out.append(("phase1a", st, pb, nb))
        elif kind == "fused":
            _, slot, rr, val, tgt = op
            out.append(("fused",) + tuple(be.phase2_fused(slot, rr, val, tgt)))
        elif kind == "k1k2":
            _, slot, rr, val, tgt, dup = op
            st0, new = be.proxy_open(slot, rr, val)
            st1, vb, nb, nr = be.acceptor_phase2a(slot, rr, val, tgt)
            st2, ch, cr, cv = be.proxy_phase2b(slot, rr, vb)
            # duplicated vote messages (10 %): delivered again, must change nothing
            idx = np.nonzero(dup)[0]
            st3, ch2, cr2, cv2 = be.proxy_phase2b(slot[idx], rr[idx], vb[idx])
            out.append(("k1k2", st0, new, st1, vb, nb, nr, st2, ch, cr, cv, st3, ch2, cr2, cv2))
        elif kind == "open":
            _, slot, rr, val = op
            out.append(("open",) + tuple(be.proxy_open(slot, rr, val)))
        elif kind == "phase2a":
            _, slot, rr, val, tgt = op
            out.append(("phase2a",) + tuple(be.acceptor_phase2a(slot, rr, val, tgt)))
        elif kind == "phase2b":
            _, slot, rr, vb = op
            out.append(("phase2b",) + tuple(be.proxy_phase2b(slot, rr, vb)))
        elif kind == "ranges":           # Mencius noop ranges, the fused step
            _, start, end, rr, tgt = op
            out.append(("ranges",) + tuple(be.noop_ranges_fused(start, end, rr, tgt)))
        elif kind == "ranges_k1k2":       # the same in its three unfused calls, the tally fed with the acceptors' votes
            _, start, end, rr, tgt = op
            st0, new = be.proxy_open_noop_ranges(start, end, rr)
            st1, vb, nb, nr = be.acceptor_phase2a_noop_ranges(start, end, rr, tgt)
            st2, ch = be.proxy_phase2b_noop_ranges(start, end, rr, vb)
            out.append(("ranges_k1k2", st0, new, st1, vb, nb, nr, st2, ch))
        elif kind == "forget":
            _, first, count = op
            be.proxy_forget(first, count)
            out.append(("forget",))
        elif kind == "flush":             # lazy Phase1a promises into the cells: a no-op for a backend without records
            if hasattr(be, "flush_promises"):
                be.flush_promises()
            out.append(("flush",))
        elif kind == "p1b_scan":          # recovery: (status, max slot, safe round per slot, safe value per slot)
            _, wm, quorum, cap = op
            out.append(("p1b_scan",) + tuple(be.leader_phase1b_scan(wm, quorum, cap)))
        elif kind == "p1b_info":          # one acceptor's Phase1b.info: (slots, vote rounds, vote values)
            _, g, r, wm = op
            out.append(("p1b_info",) + tuple(be.acceptor_phase1b_info(g, r, wm)))
        elif kind == "chosen":            # the replica's log ingest: (status, executed watermark, number chosen)
            _, slot, val = op
            out.append(("chosen",) + tuple(be.replica_chosen(slot, val)))
        elif kind == "read_log":          # (values, present)
            _, first, count = op
            out.append(("read_log",) + tuple(be.replica_read_log(first, count)))
        else:
            raise ValueError(kind)
    return out


# ---- the lift: the same script at the far end of the round range and over all of int32's values ----------------------
# include/fpx.h allows rounds 0 .. MAX_ROUND and any int32 value_id.  r -> r + base on the rounds >= 0 is monotone and
# keeps -1 ("no round") lowest, a bijection on the values keeps equality: every comparison the protocol makes comes out
# the same, so run(lift(script)) == lift(run(script)) for a correct backend, whatever its key words and packed records.
MAX_ROUND = (1 << 30) - 2
INT32_MIN = -(1 << 31)
EDGE_VALUES = (INT32_MIN, INT32_MIN + 1, -2, -1, 0, (1 << 30) - 1, 1 << 30, (1 << 31) - 1)
NO_ROUND_OPS = ("forget", "flush", "p1b_scan", "p1b_info", "chosen", "read_log")
EDGE_SLOTS = (1, 2, 3, 5, 8, 13, 21, 34)   # the slots whose steady value the map sends to EDGE_VALUES, in order


class ValueMap:
    """A bijection of int32: v -> v ^ 0x80000000, followed by transpositions that make the values in `sources` (default:
    steady_values of EDGE_SLOTS) land on the literal EDGE_VALUES.  keep_noop adds one more that fixes FPX_NOOP == -1:
    scripts with Mencius noop ranges need it, since a range's vote stores -1 itself and the state cannot tell that -1
    from a command's (the edge value -1 is then carried by nobody else)."""

    def __init__(self, sources=None, keep_noop=False):
        sources = steady_values(np.array(EDGE_SLOTS)) if sources is None else sources
        self.table, inv = {}, {}
        flip = lambda x: ((int(x) + (1 << 31)) ^ (1 << 31)) % (1 << 32) - (1 << 31)    # x ^ 0x80000000 on int32
        pairs = list(zip((int(s) for s in sources), EDGE_VALUES))
        if keep_noop:
            pairs = [(s, e) for s, e in pairs if e != -1 and s != -1] + [(-1, -1)]
        assert len({s for s, _ in pairs}) == len(pairs)
        for src, dst in pairs:
            img = self.table.get(src, flip(src))        # where src goes now
            pre = inv.get(dst, flip(dst))               # who goes to dst now
            self.table[src], self.table[pre] = dst, img
            inv[dst], inv[img] = src, pre
        for src, dst in pairs:
            assert self.table[src] == dst

    def __call__(self, v):
        v = np.asarray(v, dtype=np.int32)
        out = (v.view(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
        for src, dst in self.table.items():
            out = np.where(v == src, np.int32(dst), out)
        return out.astype(np.int32)


def identity_values(v):
    return np.asarray(v, dtype=np.int32)


def lift_rounds(r, base):
    """rounds >= 0 move up by base; -1 (no round) stays"""
    if r is None:
        return None
    if np.ndim(r) == 0:
        return int(r) + base if int(r) >= 0 else int(r)
    r = np.asarray(r, dtype=np.int64)
    out = np.where(r >= 0, r + base, r)
    assert out.max(initial=0) <= MAX_ROUND
    return out.astype(np.int32)


def lift_values(v, present, vmap):
    """vmap where `present` (a bool array, or True for everywhere) says a value is there"""
    v = np.asarray(v, dtype=np.int32)
    return np.where(present, vmap(v), v).astype(np.int32)


def script_rounds(script):
    """every round >= 0 a script carries, sorted and distinct"""
    out = set()
    for op in script:
        if op[0] in NO_ROUND_OPS:
            continue
        r = op[3] if op[0].startswith("ranges") else op[2]
        if r is not None:
            out |= {int(x) for x in np.atleast_1d(r) if x >= 0}
    return sorted(out)


def lift_bases(script):
    """the three bases every lifted test uses: `top` puts the script's highest round exactly on MAX_ROUND; `24` and `29`
    put a middle round of the script on 2^24 - 1 and 2^29 - 1, so that its rounds straddle that power of two (the last
    integer a float holds exactly; bit 29 of the 30-bit key field)"""
    rounds = script_rounds(script)
    mid = rounds[(len(rounds) - 1) // 2]
    return {"top": MAX_ROUND - rounds[-1], "24": (1 << 24) - 1 - mid, "29": (1 << 29) - 1 - mid}


def lift_script(script, base, vmap):
    out = []
    for op in script:
        kind = op[0]
        if kind == "phase1a":
            _, g, rnd, wm, tgt = op
            out.append((kind, g, lift_rounds(rnd, base), wm, tgt))
        elif kind in ("fused", "phase2a"):
            _, slot, rr, val, tgt = op
            out.append((kind, slot, lift_rounds(rr, base), vmap(val), tgt))
        elif kind == "k1k2":
            _, slot, rr, val, tgt, dup = op
            out.append((kind, slot, lift_rounds(rr, base), vmap(val), tgt, dup))
        elif kind == "open":
            _, slot, rr, val = op
            out.append((kind, slot, lift_rounds(rr, base), vmap(val)))
        elif kind == "phase2b":
            _, slot, rr, vb = op
            out.append((kind, slot, lift_rounds(rr, base), vb))
        elif kind in ("ranges", "ranges_k1k2"):
            _, start, end, rr, tgt = op
            out.append((kind, start, end, lift_rounds(rr, base), tgt))
        elif kind == "chosen":
            _, slot, val = op
            out.append((kind, slot, vmap(val)))
        elif kind in NO_ROUND_OPS:
            out.append(op)
        else:
            raise ValueError(kind)
    return out


def lift_outputs(outputs, base, vmap):
    """the outputs run_script gives for a script, as it gives them for the lifted script: Nack and Chosen rounds move (a
    -1 stays), a Chosen value is mapped where its own flag says there is one; statuses and bitmaps stay"""
    out = []
    for o in outputs:
        kind = o[0]
        if kind in ("phase1a", "open", "forget", "flush", "chosen"):
            out.append(o)
        elif kind == "p1b_scan":
            _, st, mx, sr, sv = o
            out.append((kind, st, mx, lift_rounds(sr, base), lift_values(sv, np.asarray(sr) >= 0, vmap)))
        elif kind == "p1b_info":
            _, sl, vr, vv = o
            out.append((kind, sl, lift_rounds(vr, base), lift_values(vv, True, vmap)))
        elif kind == "read_log":
            _, vals, pres = o
            out.append((kind, lift_values(vals, np.asarray(pres) == 1, vmap), pres))
        elif kind == "fused":
            _, st, ch, cr, cv, nr = o
            out.append((kind, st, ch, lift_rounds(cr, base), lift_values(cv, np.asarray(ch) == 1, vmap), lift_rounds(nr, base)))
        elif kind == "phase2a":
            _, st, vb, nb, nr = o
            out.append((kind, st, vb, nb, lift_rounds(nr, base)))
        elif kind == "phase2b":
            _, st, ch, cr, cv = o
            out.append((kind, st, ch, lift_rounds(cr, base), lift_values(cv, np.asarray(ch) == 1, vmap)))
        elif kind == "k1k2":
            _, st0, new, st1, vb, nb, nr, st2, ch, cr, cv, st3, ch2, cr2, cv2 = o
            out.append((kind, st0, new, st1, vb, nb, lift_rounds(nr, base),
                        st2, ch, lift_rounds(cr, base), lift_values(cv, np.asarray(ch) == 1, vmap),
                        st3, ch2, lift_rounds(cr2, base), lift_values(cv2, np.asarray(ch2) == 1, vmap)))
        elif kind == "ranges":
            _, st, vb, nb, nr, new, ch = o
            out.append((kind, st, vb, nb, lift_rounds(nr, base), new, ch))
        elif kind == "ranges_k1k2":
            _, st0, new, st1, vb, nb, nr, st2, ch = o
            out.append((kind, st0, new, st1, vb, nb, lift_rounds(nr, base), st2, ch))
        else:
            raise ValueError(kind)
    return out


def lift_snapshot(snap, base, vmap):
    """snapshot(be) of a backend that played a script, as it is after the lifted script: vote rounds, ballots and
    promised rounds >= 0 move, a vote's value is mapped where the cell has a vote, maxVotedSlot is a slot and stays"""
    voted = snap["vote_round"] >= 0
    return {"vote_round": lift_rounds(snap["vote_round"], base), "vote_value": lift_values(snap["vote_value"], voted, vmap),
            "ballot": lift_rounds(snap["ballot"], base), "promised": lift_rounds(snap["promised"], base),
            "max_voted": snap["max_voted"]}


def lift_tally(tally, base, vmap):
    """read_tally(slot) likewise: (round, state, value, bits) per live tally; a Pending tally (state 0) has its Phase2a's
    value, a Done one has dropped it and reads -1"""
    return [(r + base, st, int(vmap(np.array([v]))[0]) if st == 0 else v, bits) for r, st, v, bits in tally]


def assert_same_snapshot(sa, sb):
    assert sa.keys() == sb.keys()
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)


def snapshot(be):
    vr, vv, bl = be.read_state()
    pr, mv = be.read_scalars()
    return {"vote_round": vr, "vote_value": vv, "ballot": bl, "promised": pr, "max_voted": mv}


def assert_same_outputs(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and len(x) == len(y), "op %d: %s with %d outputs, %s with %d" % (k, x[0], len(x), y[0], len(y))
        for j, (u, v) in enumerate(zip(x[1:], y[1:])):
            if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v),
                                              err_msg="op %d (%s) output %d" % (k, x[0], j))
            else:
                assert u == v, "op %d (%s) output %d: %r != %r" % (k, x[0], j, u, v)


def assert_same_state(be_a, be_b, tally_slots=()):
    sa, sb = snapshot(be_a), snapshot(be_b)
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    for s in tally_slots:
        assert be_a.read_tally(int(s)) == be_b.read_tally(int(s)), "tally of slot %d" % s


# ---- EPaxos: one tick of fresh instances (used by tests/test_epaxos.py and bench_configs.py) ----------------------
def random_tick(rng, n, num_keys, m, next_number, skew, fifo=True):
    """One tick of fresh instances.  Every replica sees the tick in roughly the global order, perturbed by a
    replica-specific skew.  A leader numbers its instances in the order IT processes them
    (Replica.scala nextAvailableInstance), and with fifo=True every other replica receives one leader's
    PreAccepts in sending order (the reference's transports are TCP channels: per-pair FIFO).  fifo=False
    lets the channels reorder, which is what makes a replica meet (L, 5) before (L, 4) -- the case
    dependencies.subtractOne(instance) (Replica.scala:582) exists for."""
    leader = rng.integers(0, n, m).astype(np.int32)
    key = rng.integers(0, num_keys, m).astype(np.int32)
    is_set = (rng.random(m) < 0.5).astype(np.uint8)  # Bernoulli get/set, J/Workload.scala:75-103
    mask = np.zeros(m, np.uint8)
    others = np.array([[r for r in range(n) if r != L] for L in range(n)])   # [n][n-1]
    drop = rng.integers(0, n - 1, m)
    for j in range(n - 1):
        mask |= np.where(drop != j, 1 << others[leader, j], 0).astype(np.uint8)
    rank = np.zeros((n, m), np.int32)
    for r in range(n):
        noisy = np.arange(m) + rng.normal(0, skew, m)
        rank[r, np.argsort(noisy, kind="stable")] = np.arange(m)
    number = np.zeros(m, np.int32)
    for L in range(n):
        idx = np.nonzero(leader == L)[0]
        by_own = idx[np.argsort(rank[L, idx], kind="stable")]     # the leader's own processing order
        number[by_own] = next_number[L] + np.arange(len(idx))
        next_number[L] += len(idx)
        if fifo:
            for r in range(n):
                if r != L:   # the positions leader L's messages occupy at r, refilled in sending order
                    rank[r, by_own] = np.sort(rank[r, idx])
    return leader, number, key, is_set, mask, rank
