"""Hosted EPaxos replicas as a cluster: n contexts, each hosting one replica, exchange the frames they themselves produce under
the seeded schedules of tests/epaxos_cluster.py (drops, duplicates, silenced replicas, timers, recoveries, a heal phase), beside
a ModelCluster that gets the same messages one at a time.  Every delivered run must answer as the model does (on the first
difference the message names n, seed, fifo, the step and the receiver: tests/test_epaxos_cluster_cpu.py replays it on the model
alone); at the end the states are equal cell by cell, and EPaxos' invariants -- agreement, validity, the dependency invariant,
completion --, the command store, the key table and the execution order are checked on the contexts' own read-backs.  The seeds
and their census are those tests/test_epaxos_cluster_cpu.py holds on the CPU."""
import pytest

from tests import epaxos_cluster as C

pytestmark = pytest.mark.gpu
_default_frames = {}


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


@pytest.mark.parametrize("n,seed,fifo", sorted(C.CASES))
def test_a_cluster_of_contexts_against_the_model_and_the_invariants(wire, n, seed, fifo):
    census, frames = C.run_gpu_case(wire, n, seed, fifo)
    assert census == C.CASES[(n, seed, fifo)]
    _default_frames[(n, seed, fifo)] = frames


@pytest.mark.parametrize("n,seed,fifo", sorted(C.OTHER_FORM_CASES))
def test_word_copies_and_direct_emit_give_the_same_bytes(wire, n, seed, fifo):
    """the command store in its word-copy form and the encoder in its direct form: every frame every node emits is byte for
    byte the default forms' frame"""
    want = _default_frames.get((n, seed, fifo)) or C.run_gpu_case(wire, n, seed, fifo)[1]
    census, frames = C.run_gpu_case(wire, n, seed, fifo, env=C.OTHER_FORMS)
    assert census == C.CASES[(n, seed, fifo)]
    assert frames == want
