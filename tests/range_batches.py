"""Deterministic batches of Mencius noop ranges (plain numpy, no GPU) for the directed tests of fpx_ranges.hpp.

A batch is (start, end, round): int32 arrays of n ranges [start, end), range i of leader group start[i] % L, which
owns the slots start[i] + k L below end[i] -- rows start[i] / L ... (end[i] - 1 - start[i] % L) / L of the log.  Every
builder keeps the run contract (one round per leader group within the batch: round[i] = rounds[start[i] % L]) and
asserts what it promises, so that a case built on it cannot silently miss its target.
"""
import numpy as np

RF_JB = 8  # rows per span of k_ranges_fill_rows


def _pack(S, L, ranges, rounds):
    start = np.array([r[0] for r in ranges], np.int32)
    end = np.array([r[1] for r in ranges], np.int32)
    rounds = [0] * L if rounds is None else list(rounds)
    assert len(rounds) == L
    rnd = np.array([rounds[int(s) % L] for s in start], np.int32)
    assert (start >= 0).all() and (end >= start).all() and (end <= S).all()
    return start, end, rnd


def rows_of(start, end, L):
    """(ja, jb): first and last row of every range; jb < ja for an empty one"""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    lg = start % L
    return start // L, np.where(end > start, (end - 1 - lg) // L, start // L - 1)


def row_range(L, lg, ja, jb, extra=0):
    """the range of leader group lg over rows ja..jb; extra in [0, L) moves its end past the last slot without reaching
    the next one"""
    assert 0 <= extra < L and jb >= ja
    return ja * L + lg, jb * L + lg + 1 + extra


def band_halves(L, rows, n_ranges):
    """commands of the lower half of the leader groups (rows 0 ... 31), ranges of the upper half"""
    h = L // 2
    slot = (np.arange(32)[:, None] * L + np.arange(h)[None, :]).reshape(-1).astype(np.int32)
    ranges = [row_range(L, h + k % h, 4 * (k // h), 4 * (k // h) + k % 2, extra=k % 3) for k in range(n_ranges)]
    assert 4 * (n_ranges // h) + 2 <= rows
    start, end = (np.array(x, np.int32) for x in zip(*ranges))
    return slot, start, end


def overlaps(start, end, L):
    """bool [n]: range i shares a row with another non-empty range of its leader group (exact duplicates included)"""
    ja, jb = rows_of(start, end, L)
    lg = np.asarray(start) % L
    n = len(ja)
    out = np.zeros(n, bool)
    for i in range(n):
        if jb[i] < ja[i]:
            continue
        for k in range(n):
            if k != i and lg[k] == lg[i] and jb[k] >= ja[k] and ja[k] <= jb[i] and jb[k] >= ja[i]:
                out[i] = True
    return out


def distinct_keys(start, end, rnd):
    return len({(int(s), int(e), int(r)) for s, e, r in zip(start, end, rnd)}) == len(start)


def residue_batch(S, L, rounds=None, row_counts=(0, 1, 3, 6)):
    """ranges whose end - start takes every residue 0 ... L - 1 (mod L) at each of `row_counts` whole rows, none
    sharing a row with another; among them length 0, length 1, one row; then one that ends at S and one that starts in
    the last row"""
    rows = S // L
    nxt = [0] * L
    ranges = []
    k = 0
    for whole in row_counts:
        for d in range(L):
            lg = k % L
            k += 1
            start = nxt[lg] * L + lg
            ranges.append((start, start + whole * L + d))
            nxt[lg] += whole + (1 if d else 0) + 1   # the rows it covers, and a gap
    assert max(nxt) <= rows - 2, "the window is too short: %d rows per leader group, %d needed" % (rows, max(nxt) + 2)
    ranges.append(((rows - 2) * L + L - 1, S))        # ends at S
    ranges.append(((rows - 1) * L, (rows - 1) * L + 1))  # starts (and ends) in the last whole row
    start, end, rnd = _pack(S, L, ranges, rounds)
    length = end - start
    assert {int(x) % L for x in length} == set(range(L))
    assert 0 in length and 1 in length and ((length >= 1) & (length <= L)).any()
    ja, jb = rows_of(start, end, L)
    assert (jb[length > 0] == ((end - 1 - start % L) // L)[length > 0]).all()
    assert (np.maximum(jb - ja + 1, 0) == (length + L - 1) // L).all()      # rows = (end - start + L - 1) / L
    assert end[-2] == S and start[-1] // L == rows - 1
    assert not overlaps(start, end, L).any() and distinct_keys(start, end, rnd)
    return start, end, rnd


def overlap_batch(S, L, rounds=None, duplicates=True, first_row=0):
    """per leader group four pairs of ranges -- disjoint, touching (jb + 1 == ja'), overlapping by one row, nested --
    and, with `duplicates`, exact copies: of range 0 at the last index, and of a middle range right behind it.  Returns
    (start, end, round, dup_pairs) with dup_pairs = [(first index, later index), ...]"""
    pairs = (((0, 1), (3, 4)), ((6, 7), (8, 9)), ((11, 13), (13, 14)), ((16, 20), (17, 18)))
    assert S // L >= first_row + 22, "the window is too short"
    ranges, kind = [], []
    for lg in range(L):
        for p, (a, b) in enumerate(pairs):
            ranges.append(row_range(L, lg, first_row + a[0], first_row + a[1], extra=(lg + p) % L))
            ranges.append(row_range(L, lg, first_row + b[0], first_row + b[1], extra=(lg + 2 * p + 1) % L))
            kind += [p, p]
    ranges = [(s, min(e, S)) for s, e in ranges]
    dup_pairs = []
    if duplicates:
        mid = len(ranges) // 2
        ranges.insert(mid + 1, ranges[mid])
        kind.insert(mid + 1, kind[mid])
        dup_pairs.append((mid, mid + 1))
        ranges.append(ranges[0])
        kind.append(kind[0])
        dup_pairs.append((0, len(ranges) - 1))
    start, end, rnd = _pack(S, L, ranges, rounds)
    ja, jb = rows_of(start, end, L)
    base = [i for i in range(len(start)) if all(i != later for _, later in dup_pairs)]
    for u, v in zip(base[0::2], base[1::2]):
        assert start[u] % L == start[v] % L
        shared = min(jb[u], jb[v]) - max(ja[u], ja[v]) + 1
        if kind[u] == 0:
            assert shared < 0 and ja[v] > jb[u] + 1
        elif kind[u] == 1:
            assert jb[u] + 1 == ja[v]
        elif kind[u] == 2:
            assert shared == 1
        else:
            assert ja[u] < ja[v] and jb[v] < jb[u]
    for first, later in dup_pairs:
        assert first < later and (start[first], end[first], rnd[first]) == (start[later], end[later], rnd[later])
        assert not any((start[k], end[k]) == (start[first], end[first]) for k in range(first))
    if duplicates:
        assert dup_pairs[-1] == (0, len(start) - 1)
    ov = overlaps(start, end, L)
    assert ov.any() and not ov.all()
    return start, end, rnd, dup_pairs


def aligned_runs(L, lg_rows, rounds=None):
    """ranges whose first and last physical row on leader-group-major rows (lg * lg_rows + j) take every pair of
    alignments mod 4, with lengths of 1 ... 9 rows, none sharing a row with another"""
    S = L * lg_rows
    nxt = [0] * L
    ranges, want = [], []
    k = 0
    for a in range(4):
        for b in range(4):
            length = (b - a) % 4 + 1                  # 1 ... 4 rows
            if k % 2:
                length += 4                           # 5 ... 8
            if (a, b) == (0, 0):
                length = 9
            lg = k % L
            k += 1
            j = nxt[lg]
            while (lg * lg_rows + j) % 4 != a:
                j += 1
            ranges.append(row_range(L, lg, j, j + length - 1, extra=k % L))
            want.append((a, b))
            nxt[lg] = j + length + 1
    assert max(nxt) <= lg_rows, "%d rows per leader group needed" % max(nxt)
    ranges = [(s, min(e, S)) for s, e in ranges]
    start, end, rnd = _pack(S, L, ranges, rounds)
    ja, jb = rows_of(start, end, L)
    lg = start % L
    got = [(int((lg[i] * lg_rows + ja[i]) % 4), int((lg[i] * lg_rows + jb[i]) % 4)) for i in range(len(start))]
    assert got == want and set(got) == {(a, b) for a in range(4) for b in range(4)}
    rows = jb - ja + 1
    assert rows.min() >= 1 and rows.max() == 9 and len(set(rows.tolist())) >= 8
    assert not overlaps(start, end, L).any() and distinct_keys(start, end, rnd)
    return start, end, rnd


def span_straddlers(L, rounds=None, stride=24):
    """ranges that start or end on either side of a multiple of RF_JB = 8 rows (k_ranges_fill_rows sweeps spans of 8 rows
    from the batch's lowest row, which an anchor range pins to row 0), some across two boundaries; leader groups take
    them in turn, a leader group that gets a second one takes it `stride` rows further on"""
    shapes = ((5, 7), (5, 8), (7, 7), (7, 8), (8, 8), (8, 10), (7, 16), (8, 15), (3, 17), (15, 16))
    assert stride % RF_JB == 0 and stride > max(b for _, b in shapes)
    ranges = [(0, 1)]                                  # the anchor: leader group 0, row 0
    for k, (ja, jb) in enumerate(shapes):
        lg, lap = (k + 1) % L, (k + 1) // L
        ranges.append(row_range(L, lg, ja + lap * stride, jb + lap * stride, extra=k % L))
    S = L * span_straddlers_rows(L, stride)
    ranges = [(s, min(e, S)) for s, e in ranges]
    start, end, rnd = _pack(S, L, ranges, rounds)
    ja, jb = rows_of(start, end, L)
    assert ja.min() == 0
    sides = {(int(ja[i]) % RF_JB, "start") for i in range(1, len(ja))} | {(int(jb[i]) % RF_JB, "end") for i in range(1, len(ja))}
    assert {(7, "start"), (0, "start"), (7, "end"), (0, "end")} <= sides
    assert ((jb // RF_JB - ja // RF_JB) >= 2).any()    # some range covers a whole span and parts of two more
    assert distinct_keys(start, end, rnd)
    return start, end, rnd


def span_straddlers_rows(L, stride=24):
    """rows per leader group that span_straddlers(L) needs"""
    return ((10 + 1) // L + 1) * stride


def many_ranges(S, L, n, rounds=None, first_row=0):
    """n distinct ranges of one to three rows, n may exceed the rows of the window: leader groups in turn, every start
    row `laps` times with different ends -- so ranges of a leader group overlap once n > L x rows / 4"""
    rows = S // L - first_row
    assert rows >= 4
    ranges = []
    for k in range(n):
        lg, t = k % L, k // L
        ja = first_row + (t * 4) % (rows - 3)
        lap = (t * 4) // (rows - 3)
        assert lap < 3 * L, "the window has no room for %d distinct ranges" % n
        ranges.append(row_range(L, lg, ja, ja + lap % 3, extra=(lap // 3) % L))
    ranges = [(s, min(e, S)) for s, e in ranges]
    start, end, rnd = _pack(S, L, ranges, rounds)
    assert len(start) == n and distinct_keys(start, end, rnd)
    return start, end, rnd


def target_masks(n, A, R, f, base=0):
    """uint64 [n, A, 4]: which acceptors (bit base + r) of each acceptor group get range i -- by turns everybody and a
    bare quorum of f + 1; every third range gives one of its acceptor groups only f: that group stays below quorum and
    the range Pending"""
    out = np.zeros((n, A, 4), np.uint64)
    for i in range(n):
        for ag in range(A):
            size = f + 1 if (i + ag) % 2 else R
            if i % 3 == 0 and ag == (i // 3) % A:
                size = f
            for k in range(size):
                bit = base + (i + 2 * ag + k) % R
                out[i, ag, bit >> 6] |= np.uint64(1 << (bit & 63))
    return out
