"""tests/depgraph_ref.py -- the scipy reference the device dependency graph is held to at size -- against oracle/depgraph.py's
TarjanDependencyGraph (the port of the reference's depgraph/TarjanDependencyGraph.scala) on small graphs of every family
tests/test_depgraph_dev_components.py uses: the same executed set, the same partition into components, and the oracle's own
execution order passes the vectorised order check (which in turn refuses orders that are broken on purpose).  No GPU."""
import numpy as np
import pytest

from tests import depgraph_ref as R


def oracle_components(g, committed=None):
    from oracle import depgraph as O

    n, leader, number, first, count, deps, own_end = g
    graph = O.TarjanDependencyGraph(O.InstancePrefixSet(n))
    graph.update_executed(O.InstancePrefixSet.from_watermarks([int(f) for f in first]))
    for i in range(len(leader)):
        if committed is None or committed[i]:
            L, x = int(leader[i]), int(number[i])
            graph.commit((L, x), 0, O.InstancePrefixSet.from_epx(L, x, [int(d) for d in deps[i]], int(own_end[i])))
    comps = O.with_deep_stack(graph.execute_by_component)
    return comps[0] if isinstance(comps, tuple) else comps


def small_graphs():
    from tests.test_depgraph_dev import random_prefix_graph

    rng = np.random.default_rng(11)
    out = []
    add = lambda name, g, committed=None: out.append((name, g, committed))
    g, _ = R.stacked_ladders(rng, 60, 7)
    add("ladders", R.shuffled(rng, g))
    g, _ = R.stacked_ladders(rng, 40, 40)
    add("one ladder", g)
    deps = g[5].copy()
    deps[-1, 0] = 41                                               # the top rung names an instance beyond column 0
    add("ladders, top beyond", g[:5] + (deps,) + g[6:])
    add("ladders on four replicas", R.with_empty_column(R.stacked_ladders(rng, 30, 5)[0], 0))
    for n, m, width, jitter, p_old in [(3, 400, 12, 4, 0.0), (5, 600, 8, 3, 0.05), (7, 500, 10, 5, 0.05)]:
        g, window = R.epochs(rng, n, m, width, jitter, p_old=p_old)
        add("epochs n=%d" % n, R.shuffled(rng, g))
        for how in ("mask", "beyond"):
            g2, committed, _ = R.block_windows(rng, g, window, how)
            add("epochs n=%d, %s" % (n, how), g2, committed)
        g2, committed, _ = R.block_windows(rng, R.shifted(g, 1000 + 7 * np.arange(n)), window, "mask")
        add("epochs n=%d from other ids" % n, g2, committed)
    g, _ = R.epochs(rng, 4, 300, 8, 3, leader=np.full(300, 2))
    add("one column", g)
    g, _ = R.epochs(rng, 2, 300, 8, 3)
    add("an empty column", R.with_empty_column(g, 1))
    add("ties n=5", R.shuffled(rng, R.families_of_cycles_with_ties(20, 5)))
    add("ties n=7", R.families_of_cycles_with_ties(12, 7))
    add("ties n=3", R.families_of_cycles_with_ties(12, 3))
    for n, m, jitter in [(5, 500, 3), (3, 300, 1)]:
        leader, number, first, count, deps, own = random_prefix_graph(rng, n, m, jitter, True)
        add("random prefixes with explicit ids n=%d" % n, (n, leader, number, first, count, deps.copy(), own[:, 0]))
        late = np.arange(m) >= 9 * m // 10
        committed = ~late | (rng.random(m) > 0.03)
        far = np.nonzero(late & (rng.random(m) < 0.02))[0]
        col = (leader[far] + 1) % n
        deps[far, col] = first[col] + count[col] + rng.integers(1, 5, len(far))
        add("random prefixes with explicit ids n=%d, waiting" % n, (n, leader, number, first, count, deps, own[:, 0]), committed)
    return out


GRAPHS = small_graphs()


@pytest.mark.parametrize("name,g,committed", GRAPHS, ids=[x[0] for x in GRAPHS])
def test_reference_agrees_with_the_tarjan_oracle(name, g, committed):
    n, leader, number, first, count, deps, own_end = g
    lab, ex = R.scc_reference(*g, committed=committed)
    comps = oracle_components(g, committed)
    key = R.instance_key(leader, number)
    msg_of = {int(k): i for i, k in enumerate(key)}
    order = np.asarray([msg_of[(L << 32) | x] for c in comps for (L, x) in c], np.int64)
    comp = np.repeat(np.arange(len(comps)), [len(c) for c in comps])
    np.testing.assert_array_equal(R.canonical_of_labels(key, lab, ex), R.canonical_of_order(key, order, comp))
    assert len(comps) == len(R.component_sizes(lab, ex))
    if committed is not None:
        assert committed[ex].all()
    R.check_valid_order(n, first, count, leader, number, deps, own_end, order, comp)
    print(name, R.describe(lab, ex))


def test_order_check_refuses_what_is_wrong():
    rng = np.random.default_rng(3)
    g, _ = R.epochs(rng, 3, 400, 12, 4)
    n, leader, number, first, count, deps, own_end = g
    comps = oracle_components(g)
    key = R.instance_key(leader, number)
    msg_of = {int(k): i for i, k in enumerate(key)}
    order = np.asarray([msg_of[(L << 32) | x] for c in comps for (L, x) in c], np.int64)
    comp = np.repeat(np.arange(len(comps)), [len(c) for c in comps])
    sizes = np.asarray([len(c) for c in comps])
    assert sizes.max() >= 3 and len(comps) >= 20
    check = lambda o, c: R.check_valid_order(n, first, count, leader, number, deps, own_end, o, c)
    check(order, comp)
    with pytest.raises(AssertionError):                            # two dependent components the other way round
        blocks = [order[comp == c] for c in range(len(comps))]
        blocks[0], blocks[-1] = blocks[-1], blocks[0]              # (the last window depends on all of the first)
        check(np.concatenate(blocks), np.repeat(np.arange(len(comps)), [len(b) for b in blocks]))
    with pytest.raises(AssertionError):                            # something it depends on did not execute at all
        check(order[1:], np.maximum(comp[1:] - (sizes[0] == 1), 0))
    big = int(np.argmax(sizes))
    with pytest.raises(AssertionError):                            # a component not in (leader, id) order
        o = order.copy()
        p = np.nonzero(comp == big)[0]
        o[p[0]], o[p[1]] = o[p[1]], o[p[0]]
        check(o, comp)
    with pytest.raises(AssertionError):                            # a component cut in two: its halves name each other
        c = comp.copy()
        p = np.nonzero(comp == big)[0]
        c[p[1]:] += 1
        check(order, c)
    with pytest.raises(AssertionError):                            # a message twice
        o = order.copy()
        o[-1] = o[-2]
        check(o, comp)
    # and the partition comparison tells a merged pair of components from the true ones
    merged = np.where(comp > 3, comp - 1, comp)
    assert not np.array_equal(R.canonical_of_order(key, order, merged), R.canonical_of_order(key, order, comp))


def test_families_have_the_components_their_docstrings_promise():
    rng = np.random.default_rng(5)
    g, heights = R.stacked_ladders(rng, 3000, 40)
    lab, ex = R.scc_reference(*g)
    assert ex.all() and sorted(R.component_sizes(lab, ex).tolist()) == sorted((2 * heights).tolist())
    for n in (3, 5, 7):
        K = 300
        g = R.families_of_cycles_with_ties(K, n)
        lab, ex = R.scc_reference(*g)
        sizes = R.component_sizes(lab, ex)
        assert ex.all() and (sizes == 2).sum() == (n // 2) * K and (sizes == 1).sum() == (n // 2) * K + K and len(sizes) == (n // 2) * 2 * K + K
        # the closures are the ones the docstring states: the cycles of one k share their sum, pair by pair
        clo, _ = R.closures(g)
        two = np.nonzero(np.isin(lab, np.unique(lab)[np.unique(lab, return_counts=True)[1] == 2]))[0]
        assert sorted(np.unique(clo[two].sum(axis=1)).tolist()) == [3 * k + 2 for k in range(K)]
        # and with two and more pairs a sort on the sum alone leaves every cycle's two members apart: without the sort on the
        # closure's hash the device would cut each of them in two
        assert R.split_without_the_hash(g) == (0 if n == 3 else (n // 2) * K)


def test_the_fixed_point_needs_the_rounds_the_ladder_tests_count_on():
    """a ladder of h rungs is 2 h hops deep and a round doubles the hops covered: ceil(log2(2 h)) rounds that move something
    and the one that finds nothing to move -- 14 at the 2928 rungs and 21 at the 2^19 the device tests count chunks on"""
    for K, rounds in [(4, 4), (100, 9), (2928, 14), (3000, 14), (1 << 14, 16)]:
        g, _ = R.stacked_ladders(np.random.default_rng(0), K, 1)
        g[5][K:, 0] = np.minimum(np.arange(K) + 2, K)
        clo, r = R.closures(g)
        assert (clo[:, :2] == K).all() and r == rounds == int(np.ceil(np.log2(2 * K))) + 1
