"""An independent reference for fpx_epx_execute_dev, and the graph families tests/test_depgraph_dev_components.py feeds it.

The reference shares nothing with the device path or the host graph of csrc/fpx_depgraph.cpp: the prefix dependencies are
written out as a sparse graph and handed to scipy.  Next to the m real vertices there is one "prefix node" P(l, j) per
column position, j = 0 .. count[l], that stands for "every instance of column l below first[l] + j":
    P(l, j) -> P(l, j - 1)   and   P(l, j) -> vertex (l, j - 1)
    vertex  -> P(l, clip(w_l - first[l], 0, count[l]))  for every column l (the own column: values_end when it is set)
    vertex  -> SINK          when it is not committed, or a watermark of it lies beyond its column
A prefix node has no edge back into it from anything it reaches except through real vertices, so reachability among real
vertices is that of the materialised graph and the strongly connected components restricted to real vertices are the
components.  "Waits" is whatever reaches the sink.  tests/test_depgraph_ref.py pins this on oracle/depgraph.py's
TarjanDependencyGraph (the line-by-line port of the reference's) on small graphs of every family below."""
import numpy as np


def scc_reference(n, leader, number, first, count, deps, own_end, committed=None):
    """-> (label [m], executes [m]): the strongly connected component of every message's instance (equal labels = one
    component; the labels of waiting instances are components too), and whether it executes"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, connected_components

    m = len(leader)
    leader = np.asarray(leader, np.int64)
    number = np.asarray(number, np.int64)
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    deps, own_end = np.asarray(deps, np.int64), np.asarray(own_end, np.int64)
    assert int(count.sum()) == m
    base = np.concatenate([[0], np.cumsum(count)])[:n]
    vert = base[leader] + (number - first[leader])
    assert ((number >= first[leader]) & (number < first[leader] + count[leader])).all() and len(np.unique(vert)) == m
    pbase = m + np.concatenate([[0], np.cumsum(count + 1)])[:n]
    sink = m + int((count + 1).sum())
    blocked = np.zeros(m, bool) if committed is None else ~np.asarray(committed, bool)
    src, dst = [], []
    for l in range(n):
        w = np.where((leader == l) & (own_end > 0), own_end, deps[:, l])
        rel = w - first[l]
        blocked = blocked | (rel > count[l])
        src.append(vert), dst.append(pbase[l] + np.clip(rel, 0, count[l]))
        j = np.arange(1, count[l] + 1)
        src.append(pbase[l] + j), dst.append(pbase[l] + j - 1)
        src.append(pbase[l] + j), dst.append(base[l] + j - 1)
    src.append(vert[blocked]), dst.append(np.full(int(blocked.sum()), sink))
    src, dst = np.concatenate(src), np.concatenate(dst)
    g = sp.csr_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(sink + 1, sink + 1))
    _, lab = connected_components(g, directed=True, connection="strong")
    waits = np.zeros(sink + 1, bool)
    waits[breadth_first_order(g.T.tocsr(), sink, directed=True, return_predecessors=False)] = True
    return lab[vert], ~waits[vert]


def instance_key(leader, number):
    """one int64 per instance, for every leader and every int32 id"""
    return (np.asarray(leader, np.int64) << 32) | np.asarray(number, np.int64)


def canonical_of_labels(key, lab, ex):
    """[m]: the smallest key of the message's component where the message executes, -1 where it waits"""
    out = np.full(len(key), -1, np.int64)
    idx = np.nonzero(ex)[0]
    if len(idx):
        _, inv = np.unique(lab[idx], return_inverse=True)
        o = np.lexsort((key[idx], inv))                        # by component, then by key: each run starts with its smallest
        starts = np.nonzero(np.diff(np.concatenate([[-1], inv[o]])))[0]
        runs = np.diff(np.concatenate([starts, [len(o)]]))
        out[idx[o]] = np.repeat(key[idx[o]][starts], runs)
    return out


def canonical_of_order(key, order, comp):
    """the same from a device answer: order[p] = the message executed p-th, comp[p] = its component's number"""
    out = np.full(len(key), -1, np.int64)
    if len(order):
        k = key[order]
        starts = np.nonzero(np.diff(np.concatenate([[-1], comp])))[0]
        out[order] = np.repeat(np.minimum.reduceat(k, starts), np.diff(np.concatenate([starts, [len(k)]])))
    return out


def component_sizes(lab, ex):
    """sorted sizes of the components that execute"""
    return np.sort(np.unique(lab[ex], return_counts=True)[1]) if ex.any() else np.zeros(0, np.int64)


def describe(lab, ex):
    c = component_sizes(lab, ex)
    if not len(c):
        return "nothing executes of %d" % len(ex)
    return "executed %d of %d, components %d (singletons %d, 2-9: %d, 10-99: %d, >= 100: %d), largest %d" % (
        ex.sum(), len(ex), len(c), (c == 1).sum(), ((c > 1) & (c < 10)).sum(), ((c >= 10) & (c < 100)).sum(), (c >= 100).sum(), c.max())


def check_valid_order(n, first, count, leader, number, deps, own_end, order, comp):
    """check_valid_order of tests/test_depgraph_dev.py without a Python loop per vertex (2^20 vertices in well under a
    second): component numbers are 0, 1, .. without gaps along the order; every message is there at most once; members of a
    component are neighbours in (leader, id) order; and for every executed vertex and every column, EVERYTHING below its
    watermark there (own column: below max(watermark, values_end), which spans the vertex itself and its explicit ids) has
    executed in a component that does not come after its own -- and no watermark of it lies beyond a column"""
    leader, number = np.asarray(leader, np.int64), np.asarray(number, np.int64)
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    deps, own_end = np.asarray(deps, np.int64), np.asarray(own_end, np.int64)
    order, comp = np.asarray(order, np.int64), np.asarray(comp, np.int64)
    m = len(leader)
    assert len(order) == len(comp)
    if not len(order):
        return
    assert order.min() >= 0 and order.max() < m and len(np.unique(order)) == len(order)
    step = np.diff(comp)
    assert comp[0] == 0 and ((step == 0) | (step == 1)).all()
    key = instance_key(leader, number)[order]
    assert (np.diff(key)[step == 0] > 0).all(), "a component's members are not in (leader, id) order"
    base = np.concatenate([[0], np.cumsum(count)])[:n]
    vert = base[leader] + (number - first[leader])
    never = np.iinfo(np.int64).max
    comp_of_vertex = np.full(m, never)
    comp_of_vertex[vert[order]] = comp
    for l in range(n):
        # pm[j] = the largest component number among the column's first j instances; one that did not execute poisons it
        pm = np.concatenate([[-1], np.maximum.accumulate(comp_of_vertex[base[l]:base[l] + count[l]])])
        w = deps[order, l]
        own = leader[order] == l
        w = np.where(own, np.maximum(w, own_end[order]), w)
        rel = w - first[l]
        assert (rel <= count[l]).all(), "executed with a dependency beyond column %d" % l
        bad = pm[np.clip(rel, 0, count[l])] > comp
        assert not bad.any(), "column %d: message %d executes before something it depends on" % (l, order[np.nonzero(bad)[0][0]])


# ---------------------------------------------------------------------------------------------------------------------
# graph families: each returns (n, leader, number, first, count, deps, own_end) with the messages in the order given by
# `shuffle` (the call's answer must not depend on the order its messages are handed in)

def shuffled(rng, g):
    n, leader, number, first, count, deps, own_end = g
    p = rng.permutation(len(leader))
    return n, leader[p], number[p], first, count, deps[p], own_end[p]


def shifted(g, new_first):
    """the same graph with its columns starting at other ids"""
    n, leader, number, first, count, deps, own_end = g
    d = (np.asarray(new_first, np.int64) - first).astype(np.int64)
    deps2 = deps.astype(np.int64) + d[None, :]
    own2 = np.where(own_end > 0, own_end.astype(np.int64) + d[leader], 0)
    assert deps2.max(initial=0) < 2**31 and own2.max(initial=0) < 2**31
    return n, leader, (number.astype(np.int64) + d[leader]).astype(np.int32), np.asarray(new_first, np.int32), count, deps2.astype(np.int32), own2.astype(np.int32)


def stacked_ladders(rng, K, max_h, n=3):
    """columns 0 and 1 of K rungs each (the other columns empty), cut into segments [a, b) of random height 1 .. max_h:
    (0, x) has the watermarks (x, x + 1, 0), (1, x) has (min(x + 2, b), x, 0).  Inside a segment (1, x) -> (0, x + 1) -> (1,
    x + 1) climbs a rung per two hops and (0, x) -> (1, x) -> (0, x - 1) comes back down: each segment is exactly ONE component
    of 2 (b - a) vertices, and a segment depends on the one below it, so the order of components is forced.  The closure
    of (1, a) needs about 2 (b - a) hops.  -> graph, heights"""
    x = np.arange(K, dtype=np.int64)
    cuts = [0]
    while cuts[-1] < K:
        cuts.append(min(K, cuts[-1] + int(rng.integers(1, max_h + 1))))
    cuts = np.asarray(cuts, np.int64)
    b = cuts[np.searchsorted(cuts, x, side="right")]             # the end of x's segment
    deps = np.zeros((2 * K, n), np.int32)
    deps[:K, 0], deps[:K, 1] = x, x + 1
    deps[K:, 0], deps[K:, 1] = np.minimum(x + 2, b), x
    leader = np.repeat(np.arange(2, dtype=np.int32), K)
    number = np.tile(x, 2).astype(np.int32)
    count = np.zeros(n, np.int32)
    count[:2] = K
    return (n, leader, number, np.zeros(n, np.int32), count, deps, np.zeros(2 * K, np.int32)), np.diff(cuts)


def epochs(rng, n, m, width, jitter, leader=None, p_old=0.0):
    """m instances in proposal order, leaders random (or as given); the tick is cut into windows of random length 1 .. 2 width
    - 1.  Instance t's watermark in column l is (the column's progress when t was proposed) + a jitter in [-jitter, jitter],
    clamped to the column's progress at its window's two edges: inside a window instances name each other both ways
    (cycles), no cycle spans two windows, and every window depends on everything before it.  A share p_old of the
    instances looks old: three instances per column at most, so it is named by its window but names nothing recent.
    -> graph, window [m] (the window of every message)"""
    if leader is None:
        leader = rng.integers(0, n, m)
    leader = np.asarray(leader, np.int64)
    onehot = np.zeros((m, n), np.int64)
    onehot[np.arange(m), leader] = 1
    after = np.cumsum(onehot, axis=0)                              # the columns' progress once t is there
    prog = after - onehot
    number = prog[np.arange(m), leader]
    lens = rng.integers(1, 2 * width, m)
    ends = np.cumsum(lens)
    ends = np.minimum(ends[:np.searchsorted(ends, m) + 1], m)
    starts = np.concatenate([[0], ends[:-1]])
    window = np.repeat(np.arange(len(ends)), ends - starts)
    lo, hi = prog[starts][window], after[ends - 1][window]
    d = np.clip(prog + rng.integers(-jitter, jitter + 1, (m, n)), lo, hi)
    old = rng.random(m) < p_old
    d[old] = np.minimum(d[old], 3)
    d[np.arange(m), leader] = np.minimum(d[np.arange(m), leader], number)
    count = after[-1] if m else np.zeros(n, np.int64)
    return (n, leader.astype(np.int32), number.astype(np.int32), np.zeros(n, np.int32), count.astype(np.int32), d.astype(np.int32),
            np.zeros(m, np.int32)), window


def block_windows(rng, g, window, how, beyond_col=None):
    """makes two whole windows of the tick's last fifth wait: `how` = "mask" leaves their instances uncommitted, "beyond"
    gives each of them a watermark one or more beyond another column (beyond_col, or any but the own one).  Such a
    watermark also names EVERY instance of that column: where that column goes on into the later windows, they and the
    blocked instances are one waiting component.  -> (graph, committed or None, blocked [m])"""
    n, leader, number, first, count, deps, own_end = g
    m = len(leader)
    nw = int(window.max()) + 1
    late = np.unique(window[4 * m // 5:])
    late = late[late > window[4 * m // 5 - 1]]                      # windows that lie wholly in the last fifth
    picked = late[[len(late) // 3, 2 * len(late) // 3]]
    assert nw > 20 and len(late) >= 3
    blocked = np.isin(window, picked)
    if how == "mask":
        return g, ~blocked, blocked
    deps = deps.copy()
    idx = np.nonzero(blocked)[0]
    col = (leader[idx] + 1 + rng.integers(0, n - 1, len(idx))) % n if beyond_col is None else np.full(len(idx), beyond_col)
    assert (col != leader[idx]).all()
    end = first.astype(np.int64) + count
    deps[idx, col] = np.minimum(end[col] + rng.integers(1, 4, len(idx)), 2**31 - 1)
    return (n, leader, number, first, count, deps, own_end), None, blocked


TIE_PAIRS = {3: [(0, 1)], 5: [(0, 2), (1, 3)], 7: [(0, 5), (1, 3), (2, 4)]}


def families_of_cycles_with_ties(K, n):
    """tests/test_depgraph_dev.py's two_families_of_cycles at size, with vertices that TIE a component's closure sum and with
    families whose columns CROSS.  Columns come in pairs (a, b) = TIE_PAIRS[n]; the last column is a chain.  For every
    k < K and every pair:
        (a, 2k) and (b, k) form a cycle of two with the closure (2k + 1, k + 1) in the pair's columns;
        (a, 2k + 1), an onlooker, depends on exactly that and is depended on by the next k only: its closure is the SAME row,
        so the same sum (and the same hash), but it lies on no cycle -- only the key's `kind` keeps it out of, and behind,
        the component.
    All the pairs' cycles of one k have the same closure sum, 3k + 2, with different closures, and the pairs' columns
    interleave ((0, 2) and (1, 3); (0, 5), (1, 3) and (2, 4)): vertices are numbered column by column, so among the vertices
    of one sort key the order by vertex is a, b, a, b (n = 5) or a, b, c, b, c, a (n = 7) -- only the sort on the closure's hash
    makes a component's two members neighbours (split_without_the_hash counts the components that a sort on the key
    alone leaves apart).  In the chain every even k names k + 1 as an explicit id (values_end = k + 2: inside its own
    prefix, on no cycle -- kind 1) and every odd k names nothing recent.  Components: per pair K cycles of two and K
    singletons, and K singletons in the chain"""
    pairs = TIE_PAIRS[n]
    k = np.arange(K, dtype=np.int64)
    leader, number, deps, own = [], [], [], []
    count = np.zeros(n, np.int32)
    for a, b in pairs:
        for col, num, wa, wb in ((a, 2 * k, 2 * k, k + 1), (b, k, 2 * k + 1, k), (a, 2 * k + 1, 2 * k + 1, k + 1)):
            d = np.zeros((K, n), np.int64)
            d[:, a], d[:, b] = wa, wb
            leader.append(np.full(K, col)), number.append(num), deps.append(d), own.append(np.zeros(K, np.int64))
        count[a], count[b] = 2 * K, K
    d = np.zeros((K, n), np.int64)
    d[:, n - 1] = np.where(k % 2 == 0, k, k - 1)
    leader.append(np.full(K, n - 1)), number.append(k), deps.append(d), own.append(np.where((k % 2 == 0) & (k + 1 < K), k + 2, 0))
    count[n - 1] = K
    return (n, np.concatenate(leader).astype(np.int32), np.concatenate(number).astype(np.int32), np.zeros(n, np.int32), count,
            np.concatenate(deps).astype(np.int32), np.concatenate(own).astype(np.int32))


def closures(g):
    """-> (closure [m][n] by message, rounds): the plain fixed point the device's closure rounds compute -- c_v = cover_v v max
    over l of (the prefix max of the closures of column l below c_v[l]), every vertex at once from the round before --
    and the number of rounds, the one that moves nothing included.  Everything committed, no watermark beyond a column"""
    n, leader, number, first, count, deps, own_end = g
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    base = np.concatenate([[0], np.cumsum(count)])[:n]
    vert = base[leader] + number - first[leader]
    d = deps.astype(np.int64).copy()
    i = np.arange(len(leader))
    d[i, leader] = np.maximum(d[i, leader], own_end)
    assert (d <= first + count).all()
    clo = np.zeros_like(d)
    clo[vert] = d
    rounds = 0
    while True:
        rounds += 1
        new = clo.copy()
        for l in range(n):
            if count[l]:
                pre = np.maximum.accumulate(clo[base[l]:base[l] + count[l]], axis=0)
                j = clo[:, l] - first[l] - 1
                has = j >= 0
                new[has] = np.maximum(new[has], pre[j[has]])
        if (new == clo).all():
            return clo[vert], rounds
        clo = new


def split_without_the_hash(g):
    """how many cyclic components a sort on the closure sum alone (ties in vertex order, as a stable sort leaves them) leaves
    with members that are not neighbours: what the sort on the closure's hash is there for"""
    n, leader, number, first, count, deps, own_end = g
    lab, ex = scc_reference(*g)
    assert ex.all()
    clo, _ = closures(g)
    total = (clo - np.asarray(first, np.int64)).clip(0).sum(axis=1)
    base = np.concatenate([[0], np.cumsum(count)])[:n]
    vert = base[leader] + number - first[leader]
    _, inv, size = np.unique(lab, return_inverse=True, return_counts=True)
    cyclic = np.nonzero(size[inv] > 1)[0]                          # (the other vertices have other keys: kind 1 or 2)
    o = cyclic[np.lexsort((vert[cyclic], total[cyclic]))]
    runs = np.count_nonzero(np.diff(inv[o])) + 1
    return runs - len(np.unique(inv[cyclic]))


def with_empty_column(g, at):
    """the same graph on one replica more, whose column `at` is empty"""
    n, leader, number, first, count, deps, own_end = g
    leader2 = (leader + (leader >= at)).astype(np.int32)
    ins = lambda a: np.insert(a, at, 0, axis=a.ndim - 1)
    return n + 1, leader2, number, ins(first), ins(count), ins(deps), own_end
