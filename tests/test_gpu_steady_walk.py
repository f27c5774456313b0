"""The steady walk of the dense G = 64 vote kernels (fpx_phase2_body.inc): a chunk whose messages are all new (slot,
round)s with a free way, to uniform ballot rows whose round they are not below, stores its rows as scalars and skips
the general walk's decision.  These streams put steady and non-steady chunks into the same launch -- a known
(slot, round), a stale round (a Nack), rows made mixed by a Phase1a, rounds above the summary, a pending lazy promise,
batches that end inside a chunk -- and launches that must take the general walk (target masks, several acceptor
groups).  After every op: every output and the state digest equal the CPU oracle's, and no uniform row has a cell that
differs from its summary."""
import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_ballot_summary import Both, whole

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def check(b, slot, rnd, val, tgt=None):
    b.fused(np.asarray(slot, np.int32), whole(len(slot), rnd), np.asarray(val, np.int32), tgt)
    return b.same_state()


@pytest.mark.parametrize("R", [129, 256])
def test_steady_and_general_chunks_in_one_launch(fa, oracle, R):
    S = 8192
    b = Both(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R)
    b.phase1a(0, 0)
    b.gpu.flush_promises()
    # fresh slots in round 0, a batch that ends inside a chunk
    check(b, slot[:1003], 0, val[:1003])
    # a known (slot, round) in the middle of fresh ones: its chunk is not delivered whole
    s = np.concatenate([slot[1003:1040], [500], slot[1040:2001]])
    check(b, s, 0, W.steady_values(s))
    # above the summary: the ballot rows and their summaries move (and a batch of one chunk's worth plus one)
    check(b, slot[:600], 3, val[:600] + 1)
    check(b, slot[600:633], 3, val[600:633] + 1)
    # a stale round (row 10 is uniform in 3) inside an otherwise fresh batch: a Nack
    s = np.concatenate([slot[2001:2050], [10], slot[2050:3001]])
    check(b, s, 2, W.steady_values(s))
    # a Phase1a of some acceptors from a watermark on: the rows behind it go mixed, the ones before stay uniform
    tgt = W.bits_from_bool(W.random_subsets(rng, 1, R, R // 3, R // 3))[0]
    b.phase1a(0, 5, 4000, tgt)
    b.gpu.flush_promises()
    b.same_state()
    check(b, slot[3001:5007], 5, val[3001:5007])
    check(b, slot[3500:4500], 6, val[3500:4500] + 2)
    # a pending lazy promise (the lazy-promise kernel), then flushed, then votes above it
    b.phase1a(0, 7, 6000)
    check(b, slot[5007:7001], 7, val[5007:7001])
    b.gpu.flush_promises()
    b.same_state()
    check(b, slot[5000:S], 8, val[5000:S] + 3)
    check(b, slot[:S], 9, val[:S] + 4)
    b.close()


@pytest.mark.parametrize("R", [129, 256])
def test_launches_that_take_the_general_walk(fa, oracle, R):
    """target masks (every acceptor targeted: the same votes as a dense launch), and two acceptor groups"""
    S = 4096
    b = Both(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    b.phase1a(0, 1)
    b.gpu.flush_promises()
    everyone = W.bits_from_bool(np.ones((1500, R), bool))
    check(b, slot[:1500], 1, val[:1500], everyone)
    check(b, slot[1500:S], 1, val[1500:S])
    check(b, slot[:1500], 2, val[:1500] + 1, everyone)
    b.close()

    b = Both(fa, oracle, num_slots=S, num_replicas=R, num_groups=2, f=(R - 1) // 2, tally_ways=8)
    for g in range(2):
        b.phase1a(g, 1)
    b.gpu.flush_promises()
    check(b, slot[:2049], 1, val[:2049])
    check(b, slot[:S], 2, val[:S] + 1)
    b.close()


@pytest.mark.parametrize("R", [129, 256])
def test_unfused_k1_steady_chunks(fa, oracle, R):
    """K1 (the unfused vote kernel, whose outputs are the vote bitmaps) over uniform rows, then above them, with a stale
    message among them"""
    S = 4096
    kw = dict(num_slots=S, num_replicas=R, f=(R - 1) // 2, ballot_mode=1, tally_ways=8)
    gpu = fa.Context(fa.make_config(**kw))
    ref = oracle.System(oracle.make_config(**kw))
    slot, _, val = W.steady_stream(S)
    W.assert_same_outputs(W.run_script(gpu, [("phase1a", 0, 0, 0, None)]), W.run_script(ref, [("phase1a", 0, 0, 0, None)]))
    gpu.flush_promises()
    ops = []
    for lo, hi, r in ((0, 1003, 0), (1003, S, 0), (0, 2000, 4)):
        s = slot[lo:hi]
        ops.append(("k1k2", s, whole(len(s), r), val[lo:hi], None, np.zeros(len(s), bool)))
    s = np.concatenate([slot[2000:2100], [7], slot[2100:3001]]).astype(np.int32)
    ops.append(("k1k2", s, whole(len(s), 3), W.steady_values(s), None, np.zeros(len(s), bool)))
    for op in ops:
        W.assert_same_outputs(W.run_script(gpu, [op]), W.run_script(ref, [op]))
        uniform, mixed, bad = gpu.ballot_summary_audit()
        assert bad == 0 and uniform + mixed == S
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, 61))
    gpu.close()
