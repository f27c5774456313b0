"""The vote-row records of FPX_BALLOT_PER_SLOT at more than 128 acceptors per group (State::vote_sum, row state
ROW_COMPACT): a chunk in which the whole group votes (the steady walk of the dense G = 64 vote kernel) stores one
(round, value) record per row instead of 2 x R cells; every reader of a cell takes the record; a vote that does not come
from the whole group first writes the record into every cell.

Every script runs on the CPU oracle and on TWO GPU contexts, because the cell readback (fpx_read_state) turns every
compact row back into cells: `gpu` keeps its compact rows from op to op -- after every op its outputs, its state digest
(which reads compact rows through their records) and its row-state counts (fpx_vote_summary_audit, against the counts the
script expects: a run in which no row ever went compact fails) are checked, and at the end of the script its cells; `twin`
is read back after every op, cell by cell, so its rows are expanded again and again and meet the next op as cells."""
import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_ballot_summary import whole

pytestmark = pytest.mark.gpu

PER_SLOT, ACCEPTOR = 1, 0
S = 4096


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def chunk_for(n, cus):
    """messages per wavefront of a vote launch in a context that keeps records (fpx_api.hip, chunk_for): 64 when that
    fills the chip with 16 wavefronts per CU, else halved down to 4"""
    ch = 64
    while ch > 4 and (n + ch - 1) // ch < cus * 16:
        ch >>= 1
    return ch


class Rows:
    def __init__(self, fa, oracle, ballot_mode=PER_SLOT, twin=True, **kw):
        kw = dict(kw, ballot_mode=ballot_mode, tally_ways=8)
        self.gpu = fa.Context(fa.make_config(**kw))
        self.twin = fa.Context(fa.make_config(**kw)) if twin else None
        self.ref = oracle.System(oracle.make_config(**kw))
        self.S, self.R, self.per_slot = kw["num_slots"], kw["num_replicas"], ballot_mode == PER_SLOT

    def call(self, name, *args):
        """one op on the three backends; both GPU contexts must answer what the oracle answers"""
        want = getattr(self.ref, name)(*args)
        for be in self.contexts():
            got = getattr(be, name)(*args)
            if want is None:
                continue
            assert len(got) == len(want)
            for j, (x, y) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg="%s output %d" % (name, j))
        return want

    def contexts(self):
        return (self.gpu, self.twin) if self.twin else (self.gpu,)

    def setup(self, rnd=0, groups=1):
        for g in range(groups):
            self.call("acceptor_phase1a", g, rnd, 0, None)
        self.flush()

    def flush(self):
        for be in self.contexts():
            be.flush_promises()

    def check(self, want):
        """after an op: `want` = (fresh, cells, compact) rows of `gpu`"""
        assert self.gpu.vote_summary_audit() == want
        if self.per_slot:
            for be in self.contexts():
                uniform, mixed, bad = be.ballot_summary_audit()
                assert bad == 0 and uniform + mixed == self.S
        np.testing.assert_array_equal(self.gpu.state_digest(), self.ref.state_digest())
        assert self.gpu.vote_summary_audit() == want, "a digest must leave the records as they are"
        if self.twin:
            np.testing.assert_array_equal(self.twin.state_digest(), self.ref.state_digest())
            self.same_cells(self.twin)
            assert self.twin.vote_summary_audit()[2] == 0

    def same_cells(self, be):
        for x, y, what in zip(be.read_state(), self.ref.read_state(), ("vote_round", "vote_value", "ballot")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        for x, y in zip(be.read_scalars(), self.ref.read_scalars()):
            np.testing.assert_array_equal(x, y)

    def fused(self, want, slot, rnd, val, tgt=None):
        slot = np.asarray(slot, np.int32)
        self.call("phase2_fused", slot, whole(len(slot), rnd), np.asarray(val, np.int32), tgt)
        self.check(want)

    def finish(self):
        """the cells of `gpu` itself: every compact row is written out"""
        fresh, cells, compact = self.gpu.vote_summary_audit()
        self.same_cells(self.gpu)
        assert self.gpu.vote_summary_audit() == (fresh, cells + compact, 0)
        np.testing.assert_array_equal(self.gpu.state_digest(), self.ref.state_digest())
        for be in self.contexts():
            be.close()


def readers(b, watermark):
    """every reader of vote cells, on the three backends, against the oracle (or its cells where it has no such call)"""
    S, R = b.S, b.R
    before = b.gpu.vote_summary_audit()
    vr, vv, _ = b.ref.read_state()
    # the recovery scan with a quorum that leaves out acceptor 0: the arg-max must come from the quorum's lowest member
    quorum = np.ones((1, R), bool)
    quorum[0, 0] = False
    b.call("leader_phase1b_scan", watermark, W.bits_from_bool(quorum), S)
    b.call("leader_phase1b_scan", 0, W.bits_from_bool(quorum), S)
    for r in (0, R - 1):
        sl, ivr, ivv = b.call("acceptor_phase1b_info", 0, r, watermark)
        keep = np.nonzero(vr[watermark:, r] >= 0)[0] + watermark
        np.testing.assert_array_equal(sl, keep)
        np.testing.assert_array_equal(ivr, vr[keep, r])
        np.testing.assert_array_equal(ivv, vv[keep, r])
    # Phase1b.info of everybody: entry e owns the records of acceptor e, slots ascending
    voted = (vr >= 0).T.copy()
    voted[:, :watermark] = False
    e_idx, s_idx = np.nonzero(voted)
    off = np.concatenate([[0], np.cumsum(voted.sum(1))])
    for be in b.contexts():
        goff, gsl, gvr, gvv = be.acceptor_phase1b_info_all(watermark)
        np.testing.assert_array_equal(goff, off)
        np.testing.assert_array_equal(gsl, s_idx)
        np.testing.assert_array_equal(gvr, vr[s_idx, e_idx])
        np.testing.assert_array_equal(gvv, vv[s_idx, e_idx])
        for r in (0, R - 1):
            for first, count in ((0, S), (0, 1), (watermark, 777), (S - 65, 65), (1500, 300)):
                hit = np.nonzero(vr[first:first + count, r] >= 0)[0]
                assert be.acceptor_max_voted_in(0, r, first, count) == (first + hit.max() if len(hit) else -1)
            p, m, avr, avv, _ = b.ref.read_acceptor(0, r)
            got = be.read_acceptor(0, r)
            np.testing.assert_array_equal(got[2], avr)
            np.testing.assert_array_equal(got[3], avv)
    assert b.gpu.vote_summary_audit() == before, "no reader turns a record into cells"


@pytest.mark.parametrize("R", [129, 256])
def test_compact_then_read(fa, oracle, R):
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2)
    slot, _, val = W.steady_stream(S)
    b.setup()
    b.check((S, 0, 0))
    b.fused((S - 1, 0, 1), slot[:1], 0, val[:1])                # one workgroup that finalises itself
    b.fused((S - 1004, 0, 1004), slot[1:1004], 0, val[1:1004])  # a batch that ends inside a chunk
    b.fused((0, 0, S), slot[1004:], 0, val[1004:])
    readers(b, 100)
    b.check((0, 0, S))
    b.finish()


@pytest.mark.parametrize("delivery", ["scattered", "runs"])
@pytest.mark.parametrize("R", [129, 256])
def test_a_partial_vote_expands_the_row(fa, oracle, R, delivery):
    """thrifty delivery to f + 1 acceptors of compact rows, in a higher round: at random with FPX_F_SCATTERED_TARGETS
    (MODE 2), to runs of neighbours without it (MODE 1; at R = 256 behind the packed walk, which takes fresh rows only
    and leaves these chunks alone).  The cells nobody votes in get the row's record"""
    f = (R - 1) // 2
    flags = fa.FPX_F_SCATTERED_TARGETS if delivery == "scattered" else 0
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=f, flags=flags)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R)
    b.setup()
    b.fused((0, 0, S), slot, 0, val)
    subsets = W.random_subsets if delivery == "scattered" else W.run_subsets
    tgt = W.bits_from_bool(subsets(rng, 1000, R, f + 1, f + 1))
    b.fused((0, 1000, S - 1000), slot[1000:2000], 2, val[1000:2000] + 1, tgt)
    readers(b, 900)
    # fewer than a quorum in round 1, over cell rows (whose voters of round 2 Nack) and compact ones: tallies stay pending
    tgt = W.bits_from_bool(subsets(rng, 300, R, 3, f))
    b.fused((0, 1100, S - 1100), slot[1800:2100], 1, val[1800:2100] + 2, tgt)
    b.check((0, 1100, S - 1100))
    b.finish()


@pytest.mark.parametrize("R", [129, 256])
def test_expansion_with_nobody_voting(fa, oracle, R):
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2)
    slot, _, val = W.steady_stream(S)
    b.setup()
    b.fused((0, 0, S), slot, 0, val)
    # round 5 is promised from slot 2050 on; the batch's chunks start at multiples of their size from slot 1024, so the
    # chunk that starts at 2048 holds rows of both kinds (the general walk: its first two rows are voted by everybody and
    # leave as cells), every chunk before it is steady and every row behind it Nacks in every cell
    b.call("acceptor_phase1a", 0, 5, 2050, None)
    b.flush()
    b.check((0, 0, S))
    b.fused((0, 1024, S - 1024), slot[1024:3072], 3, val[1024:3072] + 7)
    vr, vv, _ = b.ref.read_state()
    assert (vr[1024:2050] == 3).all() and (vr[2050:3072] == 0).all() and (vv[2050:3072] == val[2050:3072, None]).all()
    b.finish()


@pytest.mark.parametrize("R", [129, 256])
def test_compact_again(fa, oracle, R, cus):
    f = (R - 1) // 2
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=f)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R + 1)
    b.setup()
    b.fused((0, 0, S), slot, 0, val)
    part = np.array([10, 11, 12, 13, 2000, 2001, 2002], np.int32)
    b.fused((0, 7, S - 7), part, 1, W.steady_values(part) + 1, W.bits_from_bool(W.random_subsets(rng, 7, R, f + 1, f + 1)))
    # everybody votes in those rows, but their ballot rows are mixed: the general walk, cells again, ballots uniform in 2
    b.fused((0, 7, S - 7), part, 2, W.steady_values(part) + 2)
    b.fused((0, 6, S - 6), [2001], 3, [5])                      # steady by now; (2001, 3) is known from here on
    # rows 0 .. 1022 in round 3, the known (2001, 3) in the middle: the chunk that holds it is not steady -- its other
    # rows get cells from the whole group's votes, row 2001 is left as it is -- and every other chunk goes compact, the
    # one with the cell rows 10 .. 13 among compact ones included
    s = np.concatenate([slot[:500], [2001], slot[500:1023]]).astype(np.int32)
    ch = chunk_for(len(s), cus)
    cells = (ch - 1) + 2                                        # that chunk's other rows; 2000 and 2002
    b.fused((0, cells, S - cells), s, 3, W.steady_values(s) + 3)
    b.fused((0, 2, S - 2), slot[:1023], 4, val[:1023])
    b.finish()


@pytest.mark.parametrize("R", [129, 256])
def test_recycled_rows_are_fresh(fa, oracle, R):
    f = (R - 1) // 2
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=f)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R + 2)
    b.setup()
    b.fused((0, 0, S), slot, 0, val)
    b.call("proxy_forget", 0, 100)                              # tallies only: the rows keep their records
    b.check((0, 0, S))
    b.fused((0, 0, S), slot[:100], 1, val[:100] + 1)
    b.call("recycle_slots", 1000, 500)
    b.check((500, 0, S - 500))
    # thrifty delivery to runs of fresh rows (at R = 256 the packed walk): whole cells blended with the -1 they must hold
    tgt = W.bits_from_bool(W.run_subsets(rng, 400, R, f + 1, f + 1))
    b.fused((100, 400, S - 500), slot[1000:1400], 1, val[1000:1400] + 3, tgt)
    tgt = W.bits_from_bool(W.random_subsets(rng, 50, R, f + 1, f + 1))
    b.fused((50, 450, S - 500), slot[1400:1450], 1, val[1400:1450] + 3, tgt)
    b.fused((0, 450, S - 450), slot[1450:1500], 1, val[1450:1500])
    b.finish()


@pytest.mark.parametrize("R", [129, 256])
def test_pending_lazy_promise_over_compact_rows(fa, oracle, R):
    b = Rows(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2)
    slot, _, val = W.steady_stream(S)
    b.setup()
    b.fused((0, 0, S), slot, 0, val)
    b.call("acceptor_phase1a", 0, 7, 2050, None)                # pending: the lazy-promise kernels walk every chunk
    b.fused((0, 2048, S - 2048), slot[1024:3072], 7, val[1024:3072] + 1)
    b.fused((0, 2048 + 40, S - 2048 - 40), slot[3072:3112], 3, val[3072:3112] + 2)   # stale behind the promise: all Nack
    b.flush()
    b.check((0, 2048 + 40, S - 2048 - 40))
    b.fused((0, 1024, S - 1024), slot[2048:], 8, val[2048:] + 3)
    b.fused((0, 0, S), slot, 9, val + 4)
    b.finish()


@pytest.mark.parametrize("R,groups,mode", [(128, 1, PER_SLOT), (256, 2, PER_SLOT), (256, 1, ACCEPTOR)])
def test_contexts_that_keep_no_records(fa, oracle, R, groups, mode):
    f = (R - 1) // 2
    b = Rows(fa, oracle, ballot_mode=mode, num_slots=S, num_replicas=R, num_groups=groups, f=f)
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R + groups + mode)
    for g in range(groups):
        b.call("acceptor_phase1a", g, 1, 0, None)
    b.flush()
    b.check((S, 0, 0))
    b.fused((S - 1003, 1003, 0), slot[:1003], 1, val[:1003])
    b.fused((0, S, 0), slot[1003:], 1, val[1003:])
    tgt = W.bits_from_bool(W.random_subsets(rng, 1000, R, f + 1, f + 1))
    b.fused((0, S, 0), slot[1000:2000], 2, val[1000:2000] + 1, tgt)
    b.fused((0, S, 0), slot, 3, val + 2)
    b.call("recycle_slots", 64, 300)
    b.check((300, S - 300, 0))
    b.finish()


def test_the_headline_chunk_size(fa, oracle, cus):
    """64 messages per wavefront, which only a batch that fills the chip gets: one steady batch a few messages above
    that bound, then a thrifty batch over some of its rows (64 messages: four per wavefront), then the general walk at
    64 messages per wavefront over compact rows: a dense batch of the same size whose rows behind a promised watermark
    Nack in every cell and are written out.  (At this size the cells are read back once, at the end, and there is no
    second context)"""
    R, f = 256, 127
    n = 64 * 16 * cus + 37
    assert chunk_for(n, cus) == 64 and chunk_for(64 * 16 * cus - 64, cus) == 32
    b = Rows(fa, oracle, twin=False, num_slots=n + 64, num_replicas=R, f=f)
    slot, _, val = W.steady_stream(n + 64)
    rng = np.random.default_rng(5)
    b.setup()
    b.fused((64, 0, n), slot[:n], 0, val[:n])
    at = n - 50                                                 # the batch's last, partial chunk and the one before it
    tgt = W.bits_from_bool(W.random_subsets(rng, 64, R, f + 1, f + 1))
    b.fused((50, 64, n - 50), slot[at:at + 64], 2, val[at:at + 64] + 1, tgt)
    # round 5 is promised from slot 64 K + 2 on.  The batch's chunks start at multiples of 64: those before 64 K are
    # steady and stay compact with the new record; the one at 64 K holds rows of both kinds and takes the general walk
    # (its first two rows are voted by everybody and leave as cells); every row behind it Nacks in every cell, so its
    # record (or, in the 50 rows of the thrifty batch, its cells) must survive in all of them
    K = n // 64 - 40
    b.call("acceptor_phase1a", 0, 5, 64 * K + 2, None)
    b.flush()
    b.check((50, 64, n - 50))
    b.fused((50, n - 64 * K + 14, 64 * K), slot[:n], 3, val[:n] + 7)
    b.finish()
