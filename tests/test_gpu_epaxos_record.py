"""kp_pack / kp_unpack (frankenpaxos_amd/csrc/fpx_epaxos_rec.hpp), the record every command of a second-form EPaxos tick
crosses HBM as, packed and unpacked on the GPU by the test-only harness tests/epaxos_record_harness.hip: the round trip is
exact at the top bit of every field -- index and ranks of 2^20 and 2^21 - 1 (2^21 - 2: the largest rank of the largest
tick), the third rank's two 11-bit halves either side of 2047 / 2048, every leader, every legal resp_mask and seen_mask."""
import numpy as np
import pytest

from tests import epaxos_record as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [3, 5, 7])
def test_records_round_trip_exactly(n):
    import torch

    dev = torch.device("cuda:0")
    fields, ranks = R.records(n)
    count = len(fields[0])
    assert 3000 < count < 6000
    # the cases the records must contain
    i, x, L, is_set, resp, seen = fields
    assert set(R.INDICES) <= set(i.tolist()) and set(R.NUMBERS) <= set(x.tolist()) and set(L.tolist()) == set(range(n))
    assert {(a, b, c, d) for a, b, c, d in zip(L.tolist(), resp.tolist(), seen.tolist(), is_set.tolist())} >= \
        {(a, b, c, d) for (a, b, c) in R.headers(n) for d in (0, 1)}
    assert len(R.headers(n)) == 2 * n * (n - 1)
    for q in range(n):
        assert set(R.RANKS) <= set(ranks[q].tolist())
    lib = R.lib()
    ni = lib.er_record_words(n)
    assert ni == {3: 4, 5: 6, 7: 8}[n]
    d = [torch.from_numpy(a).to(dev) for a in fields] + [torch.from_numpy(ranks).to(dev)]
    words = torch.zeros((count, ni), dtype=torch.int32, device=dev)
    out = [torch.full((count,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    ork = torch.full((n, count), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.er_round_trip(n, count, *[t.data_ptr() for t in d], words.data_ptr(), *[t.data_ptr() for t in out],
                             ork.data_ptr()) == 0
    oi, ox, oflags = (t.cpu().numpy() for t in out)
    np.testing.assert_array_equal(oi, i)
    np.testing.assert_array_equal(ox, x)
    np.testing.assert_array_equal(oflags, L | (is_set << 3) | (resp << 8) | (seen << 16))
    np.testing.assert_array_equal(ork.cpu().numpy(), ranks)
    # the record's first words as fpx_epaxos_kp.hpp documents them: n <= 5 the index under a header, n = 7 the plain index
    w = words.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(w[:, 0] & ((1 << 21) - 1) if n <= 5 else w[:, 0], i.astype(np.uint32))
    np.testing.assert_array_equal(w[:, 1], x.astype(np.uint32))
