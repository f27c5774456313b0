"""The steady front pass of the dense G = 64 vote kernels (fpx_phase2_body.inc): a wavefront asks for its chunk's
messages and the abort flag together, then for the rows' summaries and key rows, and decides the chunk in front of the
unit loop: a steady chunk leaves records and its outputs straight from registers, any other is handed to the general walk
untouched and loaded again there, whatever its neighbours in the workgroup do.  The sizes are those of a batch that fills
the chip (64-message chunks, n >= 64 * 16 * CUs), with a partial last chunk, and one below that bound.

The batches go through the device-pointer entry points (two steps enqueued back to back are the only way to a
k_phase2_fin launch: every host call folds what is pending first), the CPU oracle gives every output, and after every
settled op the state digest and both audits are compared; cells and scalars at the end.  One context per test: at this
size a second one would double the seconds."""
import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_ballot_summary import whole

gpu = pytest.mark.gpu

CHUNK_RECORDS = 64
MAX_GRID_PER_CU = 32    # fpx_api.hip: max_grid at G = 64


# ---- the host's launch arithmetic and the kernel's two loops over it, mirrored (CPU only) -------------------------------
def chunk_for(n, cus):
    ch = CHUNK_RECORDS
    while ch > 4 and (n + ch - 1) // ch < cus * 16:
        ch >>= 1
    return ch


def grid_for(n, cus):
    ch = chunk_for(n, cus)
    nchunks = (n + ch - 1) // ch
    if nchunks <= 8:
        return 1                                   # solo
    return max(1, min((n + 4 * ch - 1) // (4 * ch), cus * MAX_GRID_PER_CU))


def wave_chunks(n, cus, grid, block, wave):
    """the (chunk, bit) pairs of one wavefront: bit k of its mask is the k-th chunk both of its loops meet"""
    ch = chunk_for(n, cus)
    nchunks = (n + ch - 1) // ch
    return [(c, k) for k, c in enumerate(range(block * 4 + wave, nchunks, grid * 4))]


@pytest.mark.parametrize("cus", [4, 256])
def test_chunk_arithmetic_around_every_boundary(cus):
    """every chunk of a batch belongs to exactly one wavefront, for n around the bound of 64-message chunks, around
    multiples of a chunk and of a workgroup, in solo launches and (few CUs) in grids capped at max_grid; a wavefront's
    mask of 64 bits covers its chunks up to 2^27 messages at 256 CUs"""
    bound = CHUNK_RECORDS * 16 * cus
    ns = {1, 7, 32, 33, 255, 256, 257}
    for base in (bound, bound + 256, bound + 5 * 256 + 64):
        ns |= {base + d for d in (-65, -64, -1, 0, 1, 37, 63, 64, 65, 255, 257)}
    if cus == 4:   # capped: several chunks per wavefront
        cap = cus * MAX_GRID_PER_CU * 256
        ns |= {cap - 1, cap, cap + 1, 2 * cap + 67, 3 * cap - 1}
    assert chunk_for(bound, cus) == 64 and chunk_for(bound - 64, cus) == 32
    for n in sorted(ns):
        ch, grid = chunk_for(n, cus), grid_for(n, cus)
        nchunks = (n + ch - 1) // ch
        owner = {}
        for block in range(grid):
            for wave in range(4):
                for c, k in wave_chunks(n, cus, grid, block, wave):
                    assert c not in owner and k < 64
                    owner[c] = (block, wave)
        assert sorted(owner) == list(range(nchunks)), n
    assert (1 << 27) // (256 * MAX_GRID_PER_CU * 4 * 64) == 64


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def up(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.view(dtype)).cuda()


class Dev:
    """one GPU context driven through the _dev entry points, and the oracle"""

    def __init__(self, fa, oracle, **kw):
        kw = dict(kw, ballot_mode=1)
        self.gpu = fa.Context(fa.make_config(**kw))
        self.ref = oracle.System(oracle.make_config(**kw))
        self.S, self.pending = kw["num_slots"], []

    def host(self, name, *args):
        want = getattr(self.ref, name)(*args)
        got = getattr(self.gpu, name)(*args)
        for j, (x, y) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg="%s output %d" % (name, j))

    def fused(self, slot, rnd, val, outs=(1, 1, 1, 1)):
        """enqueue one fused step; outs: which of chosen, chosen_round, chosen_value, nack_round are asked for"""
        import torch

        slot, val = np.asarray(slot, np.int32), np.asarray(val, np.int32)
        n = len(slot)
        want = self.ref.phase2_fused(slot, whole(n, rnd), val, None)
        assert want[0] == 0
        o = [torch.zeros(n, dtype=torch.uint8, device="cuda")] + [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
        self.gpu.phase2_fused_dev(up(slot), up(whole(n, rnd)), up(val), None, *[t if k else None for t, k in zip(o, outs)])
        self.pending.append(("fused", [t for t, k in zip(o, outs) if k], [w for w, k in zip(want[1:], outs) if k]))

    def unfused(self, slot, rnd, val):
        import torch

        slot, val = np.asarray(slot, np.int32), np.asarray(val, np.int32)
        n = len(slot)
        want = self.ref.acceptor_phase2a(slot, whole(n, rnd), val, None)
        assert want[0] == 0
        vb, nb = (torch.full((n, 4), -7, dtype=torch.int64, device="cuda") for _ in range(2))
        nr = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.gpu.acceptor_phase2a_dev(up(slot), up(whole(n, rnd)), up(val), None, vb, nb, nr)
        self.pending.append(("phase2a", [vb, nb, nr], [np.asarray(want[1]).view(np.int64), np.asarray(want[2]).view(np.int64), want[3]]))

    def settle(self, audit):
        """wait, compare every output enqueued since the last time, then the audits and the digest"""
        assert self.gpu.sync() == 0
        for name, got, want in self.pending:
            for j, (t, w) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(t.cpu().numpy(), np.asarray(w), err_msg="%s output %d" % (name, j))
        self.pending = []
        self.audits(audit)

    def audits(self, audit):
        assert self.gpu.vote_summary_audit() == audit
        uniform, mixed, bad = self.gpu.ballot_summary_audit()
        assert bad == 0 and uniform + mixed == self.S
        np.testing.assert_array_equal(self.gpu.state_digest(), self.ref.state_digest())

    def scalars(self):
        for x, y in zip(self.gpu.read_scalars(), self.ref.read_scalars()):
            np.testing.assert_array_equal(x, y)

    def finish(self):
        for x, y, what in zip(self.gpu.read_state(), self.ref.read_state(), ("vote_round", "vote_value", "ballot")):
            np.testing.assert_array_equal(x, y, err_msg=what)
        self.scalars()
        self.gpu.close()

    def forms(self):
        census = self.gpu.vote_launch_census()
        return {k[4]: v for k, v in census["cells"].items() if k[:4] == (64, 0, 1, 1)}


def big(cus):
    """the smallest batch in 64-message chunks: its chunk count is no multiple of a workgroup's four, its last chunk partial"""
    n = CHUNK_RECORDS * 16 * cus + 37
    assert chunk_for(n, cus) == 64 and ((n + 63) // 64) % 4
    return n


@gpu
@pytest.mark.parametrize("R,ways,defer", [(129, 8, True), (256, 4, True), (256, 8, False)])
def test_every_chunk_is_decided_by_itself(fa, oracle, cus, monkeypatch, R, ways, defer):
    """steady batches, then one in a higher round over the same slots with a chunk that is not steady in every wavefront
    of a workgroup and just before the partial last chunk (a known (slot, round) in it: that chunk alone leaves cells, 63
    rows, the known row untouched) and one that holds a row with a mixed ballot (everybody votes: 64 rows of cells), then two steps back to back (k_phase2_fin unless
    the fold is not deferred) with optional outputs left out"""
    if not defer:
        monkeypatch.setenv("FPX_NO_DEFER_FINALIZE", "1")
    n, f = big(cus), (R - 1) // 2
    S = n + 64
    b = Dev(fa, oracle, num_slots=S, num_replicas=R, f=f, tally_ways=ways)
    slot, _, val = W.steady_stream(S)
    b.host("acceptor_phase1a", 0, 0, 0, None)
    b.gpu.flush_promises()
    b.audits((S, 0, 0))
    # (row Y sits the first batch out: with it every slot sees four rounds, and Y a fifth -- one more than tally_ways = 4 holds)
    Y = 41 * 64 + 9
    first = np.delete(slot[:n], Y)
    b.fused(first, 0, val[first])                                      # the context's first launch: k_phase2
    b.settle((65, 0, n - 1))
    # (X_c, 2) becomes known for P slots the big batches do not hold; row Y gets a mixed ballot (f + 1 vote in round 1)
    chunks = [4 * 3 + 0, 4 * 8 + 1, 4 * 13 + 2, 4 * 18 + 3, n // 64 - 1]   # wavefront c of a workgroup; the last whole chunk
    P = len(chunks)
    X = slot[n:n + P]
    b.fused(X, 2, val[X] + 2)
    b.settle((65 - P, 0, n - 1 + P))
    at = [c * 64 + 5 for c in chunks]
    rng = np.random.default_rng(R + ways)
    tgt = W.bits_from_bool(W.random_subsets(rng, 1, R, f + 1, f + 1))
    b.host("phase2_fused", slot[Y:Y + 1], whole(1, 1), val[Y:Y + 1] + 1, tgt)
    b.audits((64 - P, 1, n - 1 + P))
    s2 = slot[:n].copy()
    s2[at] = X
    b.fused(s2, 2, W.steady_values(s2) + 2)
    cells = 63 * P + 64
    b.settle((64 - P, cells, n + P - cells))
    b.scalars()                                                        # the maxima the front pass handed on
    # back to back: chosen alone with nack_round; then everything.  Every row of the batch is uniform in round 2 by now
    b.fused(slot[:n], 3, val[:n] + 3, outs=(1, 0, 0, 1))
    b.fused(slot[:n], 4, val[:n] + 4)
    b.settle((64 - P, 0, n + P))
    forms = b.forms()
    if defer:
        assert forms.get("fin", 0) >= 1 and forms.get("fold_carried", 0) >= 1, forms
    else:
        assert "fin" not in forms and forms.get("fold_now", 0) >= 4, forms
    b.finish()


@gpu
def test_unfused_chunks_report_the_whole_group(fa, oracle, cus):
    """acceptor_phase2a_dev on a batch in 64-message chunks: the vote bitmaps, no Nack, records left behind; then a second one
    in a higher round (ballot rows and summaries from the front pass)"""
    R, n = 256, big(cus)
    S = n + 64
    b = Dev(fa, oracle, num_slots=S, num_replicas=R, f=127, tally_ways=8)
    slot, _, val = W.steady_stream(S)
    b.host("acceptor_phase1a", 0, 0, 0, None)
    b.gpu.flush_promises()
    b.unfused(slot[:n], 0, val[:n])
    b.settle((64, 0, n))
    b.unfused(slot[:n], 1, val[:n] + 1)
    b.settle((64, 0, n))
    b.scalars()
    census = b.gpu.vote_launch_census()
    assert any(k[:4] == (64, 0, 1, 0) for k in census["cells"]), census
    b.gpu.close()


@gpu
def test_an_aborted_batch_applies_nothing(fa, oracle, cus):
    """a context that validates its _dev batches: a batch with a repeated slot aborts -- the front pass asks for its
    messages before it knows, and must store nothing; the next valid batch after sync() applies fully"""
    import torch

    R, n = 256, big(cus)
    S = n + 64
    b = Dev(fa, oracle, num_slots=S, num_replicas=R, f=127, tally_ways=8)
    assert not b.gpu.cfg.flags & fa.FPX_F_TRUSTED
    slot, _, val = W.steady_stream(S)
    b.host("acceptor_phase1a", 0, 0, 0, None)
    b.gpu.flush_promises()
    b.fused(slot[:n], 0, val[:n])
    b.settle((64, 0, n))
    digest = b.gpu.state_digest()
    bad = slot[:n].copy()
    bad[70000] = bad[131]
    o = [torch.zeros(n, dtype=torch.uint8, device="cuda")] + [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    b.gpu.phase2_fused_dev(up(bad), up(whole(n, 1)), up(val[:n] + 1), None, *o)
    assert b.gpu.sync() == fa.FPX_EORDER
    assert not bool(o[0].any()) and all(bool((t == -7).all()) for t in o[1:])
    np.testing.assert_array_equal(b.gpu.state_digest(), digest)
    b.audits((64, 0, n))
    b.fused(slot[:n], 1, val[:n] + 1)
    b.settle((64, 0, n))
    b.scalars()
    b.gpu.close()


@gpu
def test_batches_in_smaller_chunks(fa, oracle, cus):
    """32 messages per wavefront (half the lanes hold no message), then 4096 messages in chunks of four"""
    n = CHUNK_RECORDS * 16 * cus - 64
    assert chunk_for(n, cus) == 32 and chunk_for(4096, cus) == 4
    b = Dev(fa, oracle, num_slots=n, num_replicas=256, f=127, tally_ways=8)
    slot, _, val = W.steady_stream(n)
    b.host("acceptor_phase1a", 0, 0, 0, None)
    b.gpu.flush_promises()
    b.fused(slot, 0, val)
    b.fused(slot[:4096], 1, val[:4096] + 1)
    b.settle((0, 0, n))
    forms = b.forms()
    assert sum(forms.get(k, 0) for k in ("solo", "grid", "fin")) == 2, forms
    b.gpu.close()
