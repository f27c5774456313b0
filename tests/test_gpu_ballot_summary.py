"""The per-row ballot summaries of FPX_BALLOT_PER_SLOT (State::ballot_sum: one round per row that every stored ballot
cell of the row holds, or "mixed"; the vote kernel does not read a row whose summary is uniform).  After every step:
no uniform row has a cell that differs from its summary (fpx_ballot_summary_audit), and every output and the whole
state equal the CPU oracle's -- a stale summary changes Nack decisions, and those show up in the outputs."""
import numpy as np
import pytest

from tests import workloads as W

pytestmark = pytest.mark.gpu

PER_SLOT = 1


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


class Both:
    """one GPU context and the oracle, driven op by op; the summaries audited after each op"""

    def __init__(self, fa, oracle, **kw):
        kw = dict(kw, ballot_mode=PER_SLOT)
        self.gpu = fa.Context(fa.make_config(**kw))
        self.ref = oracle.System(oracle.make_config(**kw))
        self.S = kw["num_slots"]

    def audit(self):
        uniform, mixed, bad = self.gpu.ballot_summary_audit()
        assert bad == 0, "%d uniform rows hold a cell that differs from their summary" % bad
        assert uniform + mixed == self.S
        return uniform, mixed

    def fused(self, slot, rnd, val, tgt=None):
        a = self.gpu.phase2_fused(slot, rnd, val, tgt)
        b = self.ref.phase2_fused(slot, rnd, val, tgt)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        return self.audit()

    def phase1a(self, group, rnd, watermark=0, tgt=None):
        a = self.gpu.acceptor_phase1a(group, rnd, watermark, tgt)
        b = self.ref.acceptor_phase1a(group, rnd, watermark, tgt)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        return self.audit()

    def recycle(self, first, count):
        self.gpu.recycle_slots(first, count)
        self.ref.recycle_slots(first, count)
        return self.audit()

    def same_state(self):
        np.testing.assert_array_equal(self.gpu.state_digest(), self.ref.state_digest())
        return self.audit()

    def close(self):
        self.gpu.close()


def whole(n, r):
    return np.full(n, r, np.int32)


def test_bench_setup_steady_reproposal_thrifty_and_lazy(fa, oracle):
    S, R = 8192, 256
    b = Both(fa, oracle, num_slots=S, num_replicas=R, f=127, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(7)
    assert b.audit() == (S, 0)                       # init: every row -1
    # the bench's setup: one Phase1a in round 0 (a lazy record), written into the cells: every row uniform in 0
    b.phase1a(0, 0)
    b.gpu.flush_promises()
    assert b.audit() == (S, 0)
    # steady steps in round 0: nothing moves, every row stays uniform
    for lo in range(0, S, S // 4):
        assert b.fused(slot[lo:lo + S // 4], whole(S // 4, 0), val[lo:lo + S // 4]) == (S, 0)
    # a re-proposal of every slot in a higher round: whole rows rewritten, uniform in round 2
    assert b.fused(slot, whole(S, 2), val + 1) == (S, 0)
    # thrifty random f + 1 in a higher round: the rows go mixed ...
    tgt = W.bits_from_bool(W.random_subsets(rng, S, R, 128, 128))
    assert b.fused(slot, whole(S, 5), val + 2, tgt)[1] == S
    # ... and a whole-group vote makes them uniform again
    assert b.fused(slot, whole(S, 6), val + 3) == (S, 0)
    # a lazy promise of round 8 over rows uniform in 6, then votes in round 8 where the promise covers them: thr == rnd
    # only through the lazy record (those cells are not rewritten); the promise is then flushed over the rest
    b.phase1a(0, 8, S // 2)
    u, m = b.fused(slot[: S // 4], whole(S // 4, 8), val[: S // 4])          # (below the watermark: cells 6 < 8)
    assert u == S
    b.fused(slot[S // 2:], whole(S // 2, 8), val[S // 2:])                     # (from the watermark on)
    b.gpu.flush_promises()
    u, m = b.same_state()
    assert u == S                                    # flushed: the promise is in the cells, every row uniform
    b.close()


def test_stale_phase1a_sweeps(fa, oracle):
    """sweep mode 2 (a Phase1a that some cells are ahead of) and mode 1 (an older lazy record below a new watermark)"""
    S, R = 4096, 256
    b = Both(fa, oracle, num_slots=S, num_replicas=R, f=127, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(11)
    b.phase1a(0, 1)
    b.fused(slot[: S // 2], whole(S // 2, 4), val[: S // 2])                 # half the rows in round 4
    # a stale Phase1a in round 3 (the voted rows are ahead): checked cell by cell, Nacked; then one in round 5
    b.phase1a(0, 3)
    b.same_state()
    b.phase1a(0, 5, S // 4, W.bits_from_bool(W.random_subsets(rng, 1, R, 100, 100))[0])
    b.same_state()
    # an older lazy record below a new watermark (mode 1): the cells of [old, new) get the older promise explicitly
    b.phase1a(0, 7, S // 8)
    b.phase1a(0, 9, S // 2)
    b.same_state()
    for r in (6, 9, 10):                             # Nacks where rows are ahead, votes elsewhere, then all vote
        tgt = W.bits_from_bool(W.random_subsets(rng, S, R, 150, 256))
        b.fused(slot, whole(S, r), val + r, tgt)
    b.fused(slot, whole(S, 11), val)
    assert b.same_state() == (S, 0)
    b.close()


def test_adversarial_stream_and_reset(fa, oracle):
    """SURVEY 8(d)'s adversarial stream (leader changes, stale Phase2a's, re-proposals, random target masks) with the
    audit after every op; then reset and recycled rows"""
    S, R = 4096, 256
    b = Both(fa, oracle, num_slots=S, num_replicas=R, f=127, tally_ways=8)
    script = W.adversarial_script(S, R, 128, 3, epochs=16, fused=True, subsets=W.fast_subsets)
    for op in script:
        W.assert_same_outputs(W.run_script(b.gpu, [op]), W.run_script(b.ref, [op]))
        b.audit()
    b.same_state()
    b.recycle(0, S // 2)                             # votes dropped, ballots kept: the summaries stay valid
    slot, _, val = W.steady_stream(S)
    b.fused(slot, whole(S, 40), val)
    assert b.same_state() == (S, 0)
    b.gpu.reset()
    b.ref.reset()
    assert b.audit() == (S, 0)
    b.same_state()
    b.close()


@pytest.mark.parametrize("R,groups,lgs", [(3, 1, 1), (3, 4, 1), (3, 1, 2), (16, 1, 1)])
def test_small_groups_keep_rows_mixed(fa, oracle, R, groups, lgs):
    """rows of at most 128 cells: no summaries are kept (the vote kernel does not read them there), the audit counts
    every row as mixed; several acceptor groups, leader-group-major rows (num_leader_groups > 1)"""
    S = 4096
    b = Both(fa, oracle, num_slots=S, num_replicas=R, num_groups=groups, num_leader_groups=lgs, f=1, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R + groups + lgs)
    for g in range(groups * lgs):
        b.phase1a(g, 1)
    b.gpu.flush_promises()
    assert b.same_state() == (0, S)
    for r in (1, 3, 2, 4):
        tgt = W.bits_from_bool(W.random_subsets(rng, S, R, 1, R))
        b.fused(slot, whole(S, r), val + r, tgt)
    b.fused(slot, whole(S, 5), val)
    assert b.same_state() == (0, S)
    b.close()


def test_replica_sharded_k1_leaves_rows_mixed(fa, oracle):
    """K1 on a replica shard (acceptors [base, base + n) of a 256-acceptor group) through the unfused entry points: a
    shard's rows are 64 cells (no summaries) and the cells are what the votes made them"""
    from frankenpaxos_amd import sharding

    S, R, world, rank = 2048, 256, 4, 1
    base, n = sharding.replica_shard(R, world, rank)
    gpu = fa.Context(fa.make_config(num_slots=S, num_replicas=n, f=127, ballot_mode=PER_SLOT, replica_base=base,
                                    replicas_total=R, tally_ways=8))
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(3)
    assert gpu.acceptor_phase1a(0, 1)[0] == 0
    gpu.flush_promises()
    assert gpu.ballot_summary_audit() == (0, S, 0)
    for r in (1, 2, 4):
        tgt = W.bits_from_bool(W.random_subsets(rng, S, R, 100, 256))
        st = gpu.acceptor_phase2a(slot, whole(S, r), val, tgt)[0]
        assert st == 0
        assert gpu.ballot_summary_audit() == (0, S, 0)
    assert gpu.acceptor_phase2a(slot, whole(S, 5), val)[0] == 0
    assert gpu.ballot_summary_audit() == (0, S, 0)
    _, _, bl = gpu.read_state()
    assert (bl == 5).all()
    gpu.close()
