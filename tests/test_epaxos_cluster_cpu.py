"""tests/epaxos_cluster.py on the CPU: ModelCluster alone on every (n, seed, fifo) the GPU test uses.  The seeds were picked
here, by search on the model alone: per n and fifo mode the fewest seeds whose union reaches every class of the census that can
occur at that n, among the seeds for which the model keeps every invariant (see test_the_reference_recovery_... for why not
every seed does) and completes within the heal bound.  The census of each seed is committed with it."""
import collections

import pytest

from tests import epaxos_cluster as C

# what cannot occur: with n = 3 the fast quorum is the slow quorum (2 of 3), so the first PreAcceptOk is alone among the "others"
# and decides on the fast path -- no disagreement, no timer; an Accept phase at n = 3 comes from recoveries only
IMPOSSIBLE = {3: {"slow_disagreement", "slow_timer"}, 5: set(), 7: set()}


@pytest.fixture(scope="module")
def runs():
    return {case: C.run_model_case(*case) for case in sorted(C.CASES)}


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_the_model_alone_keeps_every_invariant_and_completes(runs, case):
    sim, mc, bad, census = runs[case]
    assert not bad, bad[:5]
    assert sim.heal_rounds < C.HEAL_ROUNDS and sim.all_committed() and sim.pending() == 0
    assert census == C.CASES[case]
    assert sim.conflict_order is not None


@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("fifo", [True, False])
def test_the_seeds_reach_the_census_in_both_modes(n, fifo):
    reached = collections.Counter()
    for (nn, seed, ff), census in C.CASES.items():
        if (nn, ff) == (n, fifo):
            reached.update({k: v for k, v in census.items() if v})
    missing = set(C.CENSUS_KEYS) - set(reached) - IMPOSSIBLE[n] - C.SEEN_NOWHERE
    assert not missing, missing


def test_the_same_seed_gives_the_same_trace():
    case = min(C.CASES)
    a, b = C.run_model_case(*case)[0], C.run_model_case(*case)[0]
    assert a.trace == b.trace and len(a.trace) > 50


def test_every_message_survives_the_wire():
    """what the nodes put on the network, as frames of the host encoder and back through the host decoder (no GPU: the host
    half of GpuNode's path)"""
    from frankenpaxos_amd import wire

    sim = C.run_model_case(*min(C.CASES))[0]
    seen = 0
    for (_, what, r, args, got) in sim.trace:
        out = got[1]
        for dst, msg in out:
            back = C.decode_frames(wire, sim.cmds, sim.n, [C.encode_msg(wire, sim.cmds, msg)], r, dst)
            assert C._plain(back) == (msg,), (msg, back)
            seen += 1
    assert seen > 500


def test_the_checker_catches_a_fast_quorum_one_short():
    """the negative control: a ModelCluster whose fast quorum is one replica short commits on the fast path what a disjoint
    quorum never saw; the checker must report it for at least one committed seed"""
    kinds = collections.Counter()
    for case in sorted(C.CASES):
        if case[0] > 3:
            bad = C.run_model_case(*case, fast_short=True)[2]
            kinds.update(b.split(":")[0] for b in bad)
    assert kinds["agreement"] + kinds["dependency"] > 0, kinds


def test_the_reference_recovery_counts_its_own_reply_out_and_the_leaders_in():
    """KNOWN, and the reference's: handlePrepareOk (epaxos/Replica.scala:1836-1845) leaves the RECOVERING replica's PrepareOk out
    of the f matching pre-accepts, where EPaxos leaves out the instance LEADER's.  So a recovery can take the leader's own
    dependencies for chosen (n = 3: one reply is f of them) or pass over a value that f + 1 replicas with itself hold, while the
    leader, silenced meanwhile, still commits on the fast path from replies sent before the recovery.  The model and the
    kernels follow the reference (as_intended), and this seed shows the invariants broken on the model alone; the GPU cases
    use seeds where the schedule does not go there.  The checker reports which instances."""
    bad = C.run_model_case(*C.REFERENCE_RECOVERY_CASE)[2]
    kinds = collections.Counter(b.split(":")[0] for b in bad)
    assert kinds["dependency"] + kinds["agreement"] > 0 and not kinds["validity"], bad[:5]
