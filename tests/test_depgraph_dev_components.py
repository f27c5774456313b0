"""fpx_epx_execute_dev on graphs with MANY strongly connected components, against an independent reference.

tests/test_depgraph_dev.py holds the device dependency graph to the host graph, but its random graphs are one giant
component plus a few singletons, or acyclic.  What the device path rests on -- cyclic vertices grouped by equal closures
through a hash, component starts found across the 256-thread and DG_TILE edges of the sorted order, the `kind` tie-break of
one closure sum, the numbering of components, the chunks of closure rounds and what a context keeps between calls -- needs
graphs with thousands of distinct cyclic closures, deep ones, waiting ones, and odd column shapes.  The families are in
tests/depgraph_ref.py, next to the reference (scipy's strongly connected components on a graph with one node per column
prefix; tests/test_depgraph_ref.py pins it on the Tarjan oracle).  Every device answer is compared for the exact set of
executed messages, the exact partition into components, the number of components and the validity of the order; every
family also has an answer that is known without any library, which is asserted as well.  Everything is exact: integers,
sets, partitions."""
import re

import numpy as np
import pytest

from tests import depgraph_ref as R
from tests.test_depgraph_dev import dg_path  # noqa: F401  (the fixture: both forms of the closure rounds)

pytestmark = pytest.mark.gpu

BOTH = ["packed", "wide"]


def new_context(n):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, 4)


def run(epx, g, committed=None):
    """one fpx_epx_execute_dev call -> (num_executed, num_components, needs_host_path, order, component)"""
    import torch

    n, leader, number, first, count, deps, own_end = g
    m = len(leader)
    dev = torch.device("cuda:0")
    packed = np.zeros((m, epx.packed_stride()), np.int32)
    packed[:, :n] = deps
    packed[:, 2 * n] = own_end
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    order, comp = torch.full((m,), -1, dtype=torch.int32, device=dev), torch.full((m,), -1, dtype=torch.int32, device=dev)
    ne, nc, nh = epx.execute_dev(t(leader.astype(np.int32)), t(number.astype(np.int32)), t(packed), first, count, order, comp,
                                 committed=None if committed is None else t(committed.astype(np.uint8)))
    torch.cuda.synchronize()
    return ne, nc, nh, order.cpu().numpy()[:ne].astype(np.int64), comp.cpu().numpy()[:ne].astype(np.int64)


def hold_to_reference(g, out, committed=None, ref=None):
    """the device answer `out` of graph g against the reference: executed set, partition, component count, valid order.
    -> (label, executes) of the reference"""
    n, leader, number, first, count, deps, own_end = g
    ne, nc, nh, order, comp = out
    lab, ex = ref if ref is not None else R.scc_reference(*g, committed=committed)
    assert not nh
    key = R.instance_key(leader, number)
    mine, want = R.canonical_of_order(key, order, comp), R.canonical_of_labels(key, lab, ex)
    if not np.array_equal(mine, want):
        bad = np.nonzero(mine != want)[0]
        show = lambda c: "waits" if c < 0 else "component of (%d, %d)" % (c >> 32, c & 0xffffffff)
        for i in bad[:8]:
            print("message %d = instance (%d, %d): device %s, reference %s" % (i, leader[i], number[i], show(mine[i]), show(want[i])))
        assert False, "%d of %d messages differ: device executes %d in %d components, the reference %d in %d" % (
            len(bad), len(key), ne, nc, ex.sum(), len(R.component_sizes(lab, ex)))
    assert ne == ex.sum() and nc == len(R.component_sizes(lab, ex)) == (comp[-1] + 1 if ne else 0)
    R.check_valid_order(n, first, count, leader, number, deps, own_end, order, comp)
    return lab, ex


def chunk_lines(err, form):
    """FPX_DG_DEBUG's lines of one call: [(chunk, [vertices moved in round 1 .. 8], rounds enqueued)].  (The counters are not
    cleared between the chunks of a call: a later chunk's figures include the earlier ones'.)"""
    out = []
    for mt in re.finditer(r"libfpx: depgraph \((\w+)\) chunk (\d+), vertices moved per round:((?: -?\d+)+) \((\d+) rounds enqueued\)", err):
        assert mt.group(1) == form
        out.append((int(mt.group(2)), [int(x) for x in mt.group(3).split()], int(mt.group(4))))
    return out


def rounds_that_moved(chunks):
    """per chunk of one call: how many of its enqueued rounds moved something (the counters accumulate over the chunks)"""
    out, before = [], [0] * 8
    for _, moved, rounds in chunks:
        out.append(sum(1 for k in range(rounds) if moved[k] > before[k]))
        before = moved
    return out


def next_first_chunk(chunks):
    """the rounds dg_run enqueues in the first chunk of the NEXT call on the context: one more than moved something in
    this call's last chunk, at least 2, at most DG_ROUNDS = 8"""
    return max(2, min(8, rounds_that_moved(chunks)[-1] + 1))


# ---------------------------------------------------------------------------------------------------------------------
# stacked ladders

@pytest.mark.parametrize("K,max_h", [(5000, 1), (5000, 40), (20000, 3000)])
def test_stacked_ladders_are_one_component_per_segment(K, max_h, dg_path, monkeypatch, capfd):
    """R.stacked_ladders: every segment of height h is exactly one component of 2 h vertices and depends on the segment
    below it.  These seeds give: max_h 1 -- 5000 cycles of two; max_h 40 -- 251 components of 2 .. 80 vertices, 221 of them
    with 10 and more; max_h 3000 -- 13 components of 100 and more vertices, the largest 5856 (2928 rungs: a plain fixed-point
    iteration of the closures on the CPU takes 14 rounds there, the last of which moves nothing, so the call needs a second
    chunk of rounds: FPX_DG_DEBUG's lines are counted)."""
    rng = np.random.default_rng(K + max_h)
    g, heights = R.stacked_ladders(rng, K, max_h)
    g = R.shuffled(rng, g)
    monkeypatch.setenv("FPX_DG_DEBUG", "1")
    capfd.readouterr()
    out = run(new_context(3), g)
    chunks = chunk_lines(capfd.readouterr().err, dg_path)
    print("ladders K=%d max_h=%d (%s): %s" % (K, max_h, dg_path, chunks))
    lab, ex = hold_to_reference(g, out)
    assert out[0] == 2 * K and out[1] == len(heights)
    sizes = np.bincount(out[4])
    assert sorted(sizes.tolist()) == sorted((2 * heights).tolist())
    # the segments execute bottom-up: component c is the c-th segment
    assert np.array_equal(sizes, 2 * heights)
    assert {1: len(heights) == 5000, 40: len(heights) >= 200 and heights.max() >= 35,
            3000: len(heights) >= 8 and heights.max() >= 2500}[max_h]
    # a fresh context enqueues full chunks of 8: 1, 7 and 13 rounds move something (R.closures counts the same on the CPU)
    assert [c[0] for c in chunks] == list(range(len(chunks))) and all(c[2] == 8 for c in chunks)
    assert rounds_that_moved(chunks) == {1: [1], 40: [7], 3000: [8, 5]}[max_h]
    assert sum(rounds_that_moved(chunks)) + 1 == R.closures(g)[1]


def tall_ladder(K=1 << 19):
    g, heights = R.stacked_ladders(np.random.default_rng(0), K, 1)
    x = np.arange(K)
    g[5][K:, 0] = np.minimum(x + 2, K)                             # one segment: nothing cuts the climb
    return g


def test_one_ladder_of_2_to_the_19_rungs_takes_several_chunks_of_rounds(dg_path, monkeypatch, capfd):
    """One ladder of 2^19 rungs: m = 2^20 vertices, ONE component, and the closure of the bottom rung is 2^20 hops away.  A
    closure round doubles the hops covered, so the call needs about 21 rounds: dg_run's chunks 1 and 2 (DG_ROUNDS = 8 per
    chunk), with the control words cleared between them.  FPX_DG_DEBUG's lines are counted and printed: three chunks, in
    which all 8 rounds of chunks 0 and 1 and the first 4 of chunk 2 move something -- 21 rounds with the one that finds
    nothing to move, ceil(log2(2^20)) + 1, what a plain fixed-point iteration on the CPU takes as well
    (tests/test_depgraph_ref.py holds R.closures to that formula on smaller ladders)."""
    g = tall_ladder()
    monkeypatch.setenv("FPX_DG_DEBUG", "1")
    capfd.readouterr()
    out = run(new_context(3), g)
    chunks = chunk_lines(capfd.readouterr().err, dg_path)
    print("ladder of 2^19 rungs (%s): %s" % (dg_path, chunks))
    hold_to_reference(g, out)
    assert out[0] == 1 << 20 and out[1] == 1 and not out[4].any()
    assert np.array_equal(R.instance_key(g[1], g[2])[out[3]], np.sort(R.instance_key(g[1], g[2])))   # by (leader, id)
    assert [c[0] for c in chunks] == [0, 1, 2] and [c[2] for c in chunks] == [8, 8, 8] and rounds_that_moved(chunks) == [8, 8, 4]


def test_a_ladder_whose_top_rung_waits(dg_path):
    """The top rung names an instance one beyond column 0.  Stacked ladders (5000 rungs, heights up to 40): the top segment
    waits whole, everything below executes.  One ladder of full height: nothing executes -- num_executed = 0,
    num_components = 0, no error."""
    K = 5000
    rng = np.random.default_rng(7)
    g, heights = R.stacked_ladders(rng, K, 40)
    g[5][2 * K - 1, 0] = K + 1
    g = R.shuffled(rng, g)
    out = run(new_context(3), g)
    lab, ex = hold_to_reference(g, out)
    assert heights[-1] >= 2 and ex.sum() == 2 * (K - heights[-1])
    assert out[0] == 2 * (K - heights[-1]) and out[1] == len(heights) - 1
    g = tall_ladder(20000)
    g[5][-1, 0] = 20000 + 1
    out = run(new_context(3), g)
    assert out[:3] == (0, 0, 0)
    lab, ex = hold_to_reference(g, out)
    assert not ex.any()


# ---------------------------------------------------------------------------------------------------------------------
# epochs

def epochs_case(n, m, width, jitter, p_old=0.0):
    rng = np.random.default_rng(1000 * n + width + jitter)
    g, window = R.epochs(rng, n, m, width, jitter, p_old=p_old)
    return rng, g, window


# (n, m, width, jitter) -> what the reference finds for the fixed seeds, asserted as it stands: components, components of 10
# and more members, the largest component
EPOCHS = {(5, 20000, 8, 3): (4998, 838, 15), (5, 1 << 20, 40, 6): (40091, 22906, 79), (3, 20000, 200, 20): (357, 96, 392),
          (7, 20000, 30, 5): (880, 555, 59)}


@pytest.mark.parametrize("n,m,width,jitter,dg_path", [k + (f,) for k in EPOCHS for f in (BOTH if k[0] <= 5 else ["wide"])], indirect=["dg_path"])
def test_epochs_of_cycles(n, m, width, jitter, dg_path):
    """R.epochs: thousands of distinct cyclic closures, in windows that straddle every 256-vertex and DG_TILE edge of the
    sorted order.  The reference finds, for these seeds:
      (5, 20000, 8, 3)    4998 components: 2922 singletons, 1238 of 2 - 9, 838 of 10 - 15
      (5, 2^20, 40, 6)    40091 components: 14799 singletons, 2386 of 2 - 9, 22906 of 10 - 79
      (3, 20000, 200, 20) 357 components: 258 singletons, 3 of 2 - 9, 22 of 10 - 99, 74 of 100 - 392
      (7, 20000, 30, 5)   880 components: 241 singletons, 84 of 2 - 9, 555 of 10 - 59
    and everything executes.  EPOCHS is asserted on the reference's answer before the device is asked."""
    rng, g, window = epochs_case(n, m, width, jitter)
    g = R.shuffled(rng, g)
    lab, ex = R.scc_reference(*g)
    sizes = R.component_sizes(lab, ex)
    print((n, m, width, jitter), R.describe(lab, ex))
    want = EPOCHS[(n, m, width, jitter)]
    assert ex.all() and (len(sizes), (sizes >= 10).sum(), sizes.max()) == want
    hold_to_reference(g, run(new_context(n), g), ref=(lab, ex))


# the graphs of EPOCHS, one instance in twenty old-looking -> (executed, components, components of 10 and more members) of the reference
WAITING = {(5, 20000, 8, 3): (17484, 5657, 616), (5, 1 << 20, 40, 6): (915822, 90514, 19632), (3, 20000, 200, 20): (17472, 1385, 82),
           (7, 20000, 30, 5): (17519, 1835, 467)}


def waiting_case(n, m, width, jitter, how, new_first=None):
    """an epochs graph (one instance in twenty looks old) with two whole windows of its last fifth made to wait, and the
    conditions that make it worth running, from the reference alone: at least half of the tick executes, at least 1 %
    waits, and among the waiting there is a component of 10 and more members that is committed throughout, names nothing
    beyond a column, and waits only because of what it reaches"""
    rng = np.random.default_rng(1000 * n + width + jitter)
    # the last leader proposes in the first half of the tick only: a watermark beyond ITS column names nothing recent, so
    # the windows behind a blocked one are components of their own that wait for it, not one component with it
    leader = np.concatenate([rng.integers(0, n, m // 2), rng.integers(0, n - 1, m - m // 2)])
    g, window = R.epochs(rng, n, m, width, jitter, leader=leader, p_old=0.05)
    if new_first is not None:
        g = R.shifted(g, new_first(g[4]))
    g, committed, blocked = R.block_windows(rng, g, window, how, beyond_col=n - 1)
    lab, ex = R.scc_reference(*g, committed=committed)
    assert 2 * ex.sum() >= m and 100 * (~ex).sum() >= m
    innocent = ~ex & ~np.isin(lab, lab[blocked])                   # waiting components without a blocked member
    assert innocent.any() and np.unique(lab[innocent], return_counts=True)[1].max() >= 10
    late = np.arange(m) >= 4 * m // 5
    assert ex[~late].all() and ex[late].any()                       # (old-looking instances execute among the waiting ones)
    return g, committed, (lab, ex)


@pytest.mark.parametrize("how", ["mask", "beyond"])
@pytest.mark.parametrize("n,m,width,jitter,dg_path", [k + (f,) for k in WAITING for f in (BOTH if k[0] <= 5 else ["wide"])], indirect=["dg_path"])
def test_epochs_with_waiting_windows(n, m, width, jitter, how, dg_path):
    """Cycles next to waiting vertices: two whole windows of the tick's last fifth are not committed ("mask") or name an
    instance beyond a column ("beyond"); they, and every later window -- whole components that are committed throughout --
    wait because of what they reach, the old-looking instances among them execute, and so does everything before.  The
    executed set is compared exactly.  For these seeds the reference finds:
      (5, 20000, 8, 3)    17484 of 20000 execute in 5657 components (616 of 10 - 15 members)
      (5, 2^20, 40, 6)    915822 of 1048576 execute in 90514 components (19632 of 10 - 79 members)
      (3, 20000, 200, 20) 17472 of 20000 execute in 1385 components (62 of 100 - 372 members)
      (7, 20000, 30, 5)   17519 of 20000 execute in 1835 components (467 of 10 - 58 members)
    the same for "mask" and "beyond" (the same windows are blocked).  waiting_case asserts what makes a case worth running
    on the reference's answer before the device is asked."""
    g, committed, ref = waiting_case(n, m, width, jitter, how)
    print((n, m, width, jitter, how), R.describe(*ref))
    sizes = R.component_sizes(*ref)
    assert (ref[1].sum(), len(sizes), (sizes >= 10).sum()) == WAITING[(n, m, width, jitter)]
    hold_to_reference(g, run(new_context(n), g, committed), committed, ref=ref)


# ---------------------------------------------------------------------------------------------------------------------
# ties of the closure sum

@pytest.mark.parametrize("n,K,dg_path", [(5, 1024, "packed"), (5, 1024, "wide"), (3, 2100, "packed"), (3, 2100, "wide"), (7, 1024, "wide")],
                         indirect=["dg_path"])
def test_closure_sum_ties_across_tiles(n, K, dg_path):
    """R.families_of_cycles_with_ties: per column pair and k a cycle of two and an onlooker with the cycle's very closure (the
    same sum and hash; only `kind` keeps it out of the component and behind it); with two or three pairs, different
    closures with one sum, K times over, on columns that CROSS -- in vertex order the members of one key go a, b, a, b, so
    only the sort on the closure's hash makes a cycle's two members neighbours (tests/test_depgraph_ref.py asserts that a
    sort on the sum alone leaves every one of these cycles split); a chain whose even members lie inside their own
    prefix (kind 1).  m = 4 K + K
    per pair ... 7168 / 8400 / 10240 vertices: the keys cross DG_TILE positions of the sorted order.  Known answer: per
    pair K components of two and K singletons, K singletons in the chain; each cycle directly in front of its onlooker."""
    rng = np.random.default_rng(K + n)
    g = R.shuffled(rng, R.families_of_cycles_with_ties(K, n))
    m, pairs = len(g[1]), len(R.TIE_PAIRS[n])
    assert m == (3 * pairs + 1) * K >= 5120
    out = run(new_context(n), g)
    hold_to_reference(g, out)
    ne, nc, nh, order, comp = out
    assert ne == m and nc == 2 * pairs * K + K
    sizes = np.bincount(comp)
    assert (sizes == 2).sum() == pairs * K and (sizes == 1).sum() == pairs * K + K
    # every onlooker (a, 2k + 1) comes after the cycle {(a, 2k), (b, k)} whose closure it shares
    comp_of = np.empty(m, np.int64)
    comp_of[order] = comp
    leader, number = g[1], g[2]
    at = {(int(L), int(x)): int(c) for L, x, c in zip(leader, number, comp_of)}
    for a, b in R.TIE_PAIRS[n]:
        for k in range(K):
            assert at[(a, 2 * k)] == at[(b, k)] < at[(a, 2 * k + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# column shapes

def one_column_of_pairs(n, col, K):
    """every instance in column `col`: an even k names k + 1 as an explicit id (values_end = k + 2), an odd k everything below
    it: {k, k + 1} is a cycle of two for every even k"""
    k = np.arange(K)
    deps = np.zeros((K, n), np.int32)
    deps[:, col] = k
    own = np.where((k % 2 == 0) & (k + 1 < K), k + 2, 0).astype(np.int32)
    count = np.zeros(n, np.int32)
    count[col] = K
    return n, np.full(K, col, np.int32), k.astype(np.int32), np.zeros(n, np.int32), count, deps, own


@pytest.mark.parametrize("K", [255, 256, 257, 2047, 2048, 2049])
def test_ladders_on_columns_at_the_workgroup_and_tile_edges(K, dg_path):
    """stacked ladders (heights up to 40) on two columns of K = 255 .. 257 and 2047 .. 2049 instances -- a workgroup and a
    scan tile, one less, one more -- next to an EMPTY third column; then the same on five replicas with empty columns in
    front, in the middle and at the end (an empty column's tile_base / blk_base is shared with the next one's)"""
    rng = np.random.default_rng(K)
    g, heights = R.stacked_ladders(rng, K, 40)
    spread = R.with_empty_column(R.with_empty_column(g, 0), 2)
    assert spread[4].tolist() == [0, K, 0, K, 0]
    for graph in (g, spread):
        graph = R.shuffled(rng, graph)
        out = run(new_context(graph[0]), graph)
        hold_to_reference(graph, out)
        assert out[0] == 2 * K and np.array_equal(np.bincount(out[4]), 2 * heights)


@pytest.mark.parametrize("counts", [(255, 256, 257), (2047, 2048, 2049, 1, 0), (0, 2049, 0, 255, 2048), (257, 0, 0), (0, 0, 0, 0, 4097)])
def test_epochs_on_columns_of_given_lengths(counts, dg_path):
    """R.epochs (width 8, jitter 3; width 40 on one column) with the leaders dealt so that the columns have exactly these
    lengths: empty columns in front, in the middle and at the end, a column of one, everything in one column"""
    n, m = len(counts), sum(counts)
    rng = np.random.default_rng(m + n)
    leader = rng.permutation(np.repeat(np.arange(n), counts))
    g, _ = R.epochs(rng, n, m, 8, 3, leader=leader)
    assert tuple(g[4]) == counts
    lab, ex = hold_to_reference(g, run(new_context(n), g))
    sizes = R.component_sizes(lab, ex)
    print(counts, R.describe(lab, ex))
    if np.count_nonzero(counts) > 1:
        assert len(sizes) >= m // 10 and sizes.max() >= 8          # (one column alone has no cycles here: see the next test)


@pytest.mark.parametrize("n,col,K", [(3, 0, 4097), (5, 4, 4097), (5, 2, 513)])
def test_everything_in_one_column(n, col, K, dg_path):
    """one_column_of_pairs: K instances of one leader, (K - 1) / 2 cycles of two through explicit ids and one singleton"""
    g = one_column_of_pairs(n, col, K)
    out = run(new_context(n), g)
    hold_to_reference(g, out)
    assert out[0] == K and out[1] == (K + 1) // 2 and (np.bincount(out[4])[:-1] == 2).all()


def test_one_instance_and_none(dg_path):
    """m = 1: one component of one.  m = 0: the call answers FPX_OK with num_executed = num_components = 0 and touches
    nothing (the buffers may be NULL)"""
    g = one_column_of_pairs(5, 3, 1)
    out = run(new_context(5), g)
    hold_to_reference(g, out)
    assert out[:3] == (1, 1, 0) and out[3].tolist() == [0] and out[4].tolist() == [0]
    g = (5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros((0, 5), np.int32), np.zeros(0, np.int32))
    assert run(new_context(5), g)[:3] == (0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# what a context keeps between calls

def test_one_context_through_shallow_deep_and_small_ticks(dg_path, monkeypatch, capfd):
    """dg_run learns from a call how many closure rounds the next call's first chunk enqueues, and the context's buffers
    stay at the largest size seen.  One context: a shallow acyclic tick (20000 instances whose direct dependencies are
    their closures already: the first round moves nothing, so the next call starts with the smallest chunk), the ladder of
    2^19 rungs (2^20 vertices, several chunks), the shallow tick again -- the same counts and the same partition as the first
    time -- and a small cyclic tick (300 instances) behind the large one.  Every call against the reference, and
    FPX_DG_DEBUG's lines show the hint at work: a call's first chunk enqueues one round more than moved something in the
    last chunk of the call before it (2 at least: 8 on the fresh context, 2 behind the shallow tick, 3 behind the ladder,
    whose 20 moving rounds then come as 2 + 8 + 8 + 2), every later chunk 8, and over a call's chunks exactly the rounds
    of the plain fixed point move something."""
    rng = np.random.default_rng(21)
    shallow, _ = R.epochs(rng, 3, 20000, 8, 0)
    small, _ = R.epochs(rng, 3, 300, 12, 4)
    tall = tall_ladder()
    monkeypatch.setenv("FPX_DG_DEBUG", "1")
    epx = new_context(3)
    key = R.instance_key(shallow[1], shallow[2])
    answers = []
    for name, g in (("shallow", shallow), ("tall", tall), ("shallow again", shallow), ("small", small), ("shallow, a third time", shallow)):
        capfd.readouterr()
        out = run(epx, g)
        chunks = chunk_lines(capfd.readouterr().err, dg_path)
        lab, ex = hold_to_reference(g, out)
        assert ex.all()
        answers.append((out, chunks, name))
    for out, chunks, name in answers:
        print("%s (%s): %s" % (name, dg_path, chunks))
    assert answers[0][0][0] == answers[0][0][1] == 20000 and len(answers[0][1]) == 1      # acyclic, one chunk
    assert answers[1][0][:2] == (1 << 20, 1)
    expect_first = 8
    for (out, chunks, name), g in zip(answers, (shallow, tall, shallow, small, shallow)):
        assert [c[0] for c in chunks] == list(range(len(chunks))), name
        assert [c[2] for c in chunks] == [expect_first] + [8] * (len(chunks) - 1), name
        assert sum(rounds_that_moved(chunks)) + 1 == R.closures(g)[1], name
        expect_first = next_first_chunk(chunks)
    assert [c[2] for c in answers[0][1]] == [8] and rounds_that_moved(answers[0][1]) == [0]
    assert [c[2] for c in answers[1][1]] == [2, 8, 8, 8] and rounds_that_moved(answers[1][1]) == [2, 8, 8, 2]
    assert [c[2] for c in answers[2][1]] == [3] and answers[3][1][0][2] == 2
    assert len(np.unique(R.scc_reference(*small)[0])) < 300                               # the small tick has cycles
    for again in (2, 4):
        assert answers[again][0][:3] == answers[0][0][:3]
        assert np.array_equal(R.canonical_of_order(key, *answers[again][0][3:]), R.canonical_of_order(key, *answers[0][0][3:]))


# ---------------------------------------------------------------------------------------------------------------------
# instance ids

ID_END = 2**31 - 2   # include/fpx.h: first[l] + count[l] <= 2^31 - 2


@pytest.mark.parametrize("how", ["mask", "beyond"])
@pytest.mark.parametrize("where", ["2^21", "2^30", "the last ids"])
def test_columns_that_start_at_large_ids(where, how, dg_path):
    """include/fpx.h: 0 <= first[l], first[l] + count[l] <= 2^31 - 2.  An epochs tick with waiting windows (n = 5, 20000
    instances) whose columns start at 2^21, at 2^30 and END at 2^31 - 2, the last ids the contract allows -- there a
    watermark beyond the column can only be 2^31 - 1, and the cover of an instance that is not committed (the mask) has
    to lie above it as well."""
    new_first = {"2^21": lambda count: np.full(5, 1 << 21), "2^30": lambda count: (1 << 30) + 1000 * np.arange(5),
                 "the last ids": lambda count: ID_END - count.astype(np.int64)}[where]
    g, committed, ref = waiting_case(5, 20000, 8, 3, how, new_first)
    assert g[3].min() >= 1 << 21 and (where != "the last ids" or ((g[3].astype(np.int64) + g[4]) == ID_END).all())
    hold_to_reference(g, run(new_context(5), g, committed), committed, ref=ref)


def test_columns_beyond_the_id_range_are_refused(dg_path):
    """one id more than include/fpx.h allows in one column: FPX_EINVAL, not a wrong order, with and without a mask; the same
    tick one id lower runs, with the mask's windows waiting"""
    import frankenpaxos_amd as fa

    rng, g, window = epochs_case(5, 3000, 8, 3)
    for col in (0, 4):
        first = np.zeros(5, np.int64)
        first[col] = ID_END - g[4][col] + 1
        bad, committed, _ = R.block_windows(np.random.default_rng(col), R.shifted(g, first), window, "mask")
        for mask in (None, committed):
            with pytest.raises(fa.FpxError) as e:
                run(new_context(5), bad, mask)
            assert e.value.status == fa._lib.FPX_EINVAL
        first[col] -= 1
        ok = R.shifted(g, first)
        for mask in (None, committed):
            lab, ex = hold_to_reference(ok, run(new_context(5), ok, mask), mask)
            assert ex.all() == (mask is None) and ex.any()
