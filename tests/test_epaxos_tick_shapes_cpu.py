"""tests/epaxos_tick_shapes.py without a GPU: every tick it builds is a legal tick (the oracle applies it, status 0), and
has the bucket occupancy, the key sizes and the participation its name claims -- so that what
tests/test_gpu_epaxos_tick_paths.py asserts of the census is asserted of the tick it means."""
import numpy as np
import pytest

from tests import epaxos_tick_shapes as S

NS = [3, 5, 7]


def accepted(oracle, n, num_keys, tick, num_instances=0):
    a, kw = S.args(tick)
    ref = oracle.EPaxos(n, num_keys, num_instances)
    out = ref.preaccept(*a, **kw)
    assert out[0] == 0
    for row in tick[5]:
        assert (np.sort(row) == np.arange(len(row))).all()
    return out


def test_rank_rows_are_what_they_are_called():
    for n in NS:
        r = S.rank_rows("identity", n, 100)
        assert (r == np.arange(100)).all()
        r = S.rank_rows("reversed", n, 100)
        assert (r[:n - 1] == np.arange(100)).all() and (r[n - 1] == np.arange(99, -1, -1)).all()
        r = S.rank_rows("uniform", n, 1000, seed=3)
        assert all((np.sort(row) == np.arange(1000)).all() for row in r)
        assert len({row.tobytes() for row in r}) == n and not any((row == np.arange(1000)).all() for row in r)


def test_numbers_follow_each_leaders_own_order_and_masks_are_legal():
    for n in NS:
        for kind in ("identity", "reversed", "uniform"):
            for everybody in (False, True):
                nxt = [5] * n
                key = np.arange(999) % 7
                leader, number, _, _, resp, rank, seen = S.assemble(n, key, S.rank_rows(kind, n, 999, 1), everybody=everybody,
                                                                   next_number=nxt)
                for L in range(n):
                    idx = np.nonzero(leader == L)[0]
                    order = idx[np.argsort(rank[L, idx])]
                    assert number[order].tolist() == list(range(5, 5 + len(idx))) and nxt[L] == 5 + len(idx)
                assert all(bin(x).count("1") == n - 2 for x in resp) and not ((resp >> leader) & 1).any()
                assert not (resp & ~seen).any() and not ((seen >> leader) & 1).any()
                assert all(bin(x).count("1") == (n - 1 if everybody else n - 2) for x in seen)


@pytest.mark.parametrize("n", NS)
def test_one_bucket_of_24_and_of_25(oracle, n):
    for members, want in ((24, "bucket1"), (25, "bucket2")):
        t = S.one_bucket(n, 20000, members)
        accepted(oracle, n, 40, t)
        assert S.occupancy(t, 0, 1) == (members, 0, 3) and S.key_sizes(t, 40)[0] == members
        assert S.route(t, 0) == want and S.routes(t, 40) == ({"bucket1": 40} if members == 24 else {"bucket1": 39, "bucket2": 1})
        assert max(S.occupancy(t, k, 1)[0] for k in range(1, 40)) <= 2
        assert S.key_sizes(t, 40).max() <= S.LIMITS[n]["kp_tc"]


@pytest.mark.parametrize("n", NS)
def test_clumps_need_the_radix_sort(oracle, n):
    t = S.clumps(n, 20000)
    accepted(oracle, n, 40, t)
    assert S.occupancy(t, 0, 1)[0] > 24 and S.occupancy(t, 0, 2)[0] > 24 and S.routes(t, 40) == {"bucket1": 39, "radix3": 1}
    assert S.key_sizes(t, 40).max() <= S.LIMITS[n]["kp_tc"]
    if n == 7:
        t = S.clumps(7, 12000)
        accepted(oracle, 7, 40, t)
        assert S.routes(t, 40) == {"bucket1": 39, "radix2": 1} and S.key_sizes(t, 40).max() <= 640


def test_one_pass_never_and_two_passes_only_at_seven_replicas():
    """the argument of tests/test_gpu_epaxos_tick_paths.py, by enumeration of the widths: a bucket wider than 24 ranks needs
    m - 1 >= 32 NBK / 2 (the width is a power of two: 32), where the radix sort already takes ceil(bits(m) / 7) passes"""
    for n in NS:
        nbk = S.LIMITS[n]["nbk"]
        for m in list(range(1, 70)) + [127, 128, 129, 8192, 8193, 16383, 16384, 16385, (1 << 21) - 1]:
            passes = (int(m).bit_length() + 6) // 7
            if S.bucket_width(n, m) > 24:
                assert passes >= (2 if nbk == 512 else 3), (n, m)
        assert S.bucket_width(n, 16 * nbk) == 16 and S.bucket_width(n, 16 * nbk + 1) == 32


@pytest.mark.parametrize("n", NS)
def test_small_buckets_and_last_buckets(oracle, n):
    for members in (4, 5):
        t = S.many_small_buckets(n, 20480, members)
        accepted(oracle, n, 80, t)
        assert all(S.occupancy(t, k, 1)[0] == members and S.key_sizes(t, 80)[k] == members for k in range(40))
        assert (t[0][t[2] < 40] == n - 1).all()                     # the last replica leads them: it has a word of each
        for k in (0, 39):    # in slot (= message) order the last replica's ranks of a group descend
            rk = t[5][n - 1, t[2] == k]
            assert (np.diff(rk) == -1).all()
        assert S.routes(t, 80) == {"bucket1": 80} and S.key_sizes(t, 80).max() <= S.LIMITS[n]["kp_tc"]
    t = S.last_bucket(n)
    accepted(oracle, n, 40, t)
    nbk = S.LIMITS[n]["nbk"]
    assert S.occupancy(t, 0, 1) == (6, 0, nbk - 1) and S.routes(t, 40) == {"bucket1": 40}
    assert S.key_sizes(t, 40).max() <= S.LIMITS[n]["kp_tc"]
    t = S.last_bucket_second_attempt(n)
    accepted(oracle, n, 40, t)
    assert S.occupancy(t, 0, 1)[0] == 30 and S.occupancy(t, 0, 2)[0] == 2 and S.routes(t, 40) == {"bucket1": 39, "bucket2": 1}
    assert S.key_sizes(t, 40).max() <= S.LIMITS[n]["kp_tc"]
    rk = t[5][0, t[2] == 0]
    assert S.bucket_of(rk.max(), rk.min(), rk.max() - rk.min(), nbk) == nbk - 1
    assert (S.bucket_of(rk, rk.min(), rk.max() - rk.min(), nbk) == nbk - 1).sum() == 2


@pytest.mark.parametrize("n", NS)
def test_key_sizes_and_participation(oracle, n):
    counts = S.key_size_counts(n)
    L = S.LIMITS[n]
    assert counts[:5] == [0, 1, 63, 64, 65] and counts[-1] == L["kp_tc"] and counts[6] == 64 * L["kp_waves"]
    t = S.sizes(n, counts)
    accepted(oracle, n, len(counts), t)
    assert S.key_sizes(t, len(counts)).tolist() == counts
    assert S.bucket_width(n, len(t[0])) <= 24                       # no bucket can overflow: every key sorts at once
    for everybody in (False, True):
        t = S.absent_replica(n, everybody=everybody)
        accepted(oracle, n, 6, t)
        part = S.participates(t)
        k0 = t[2] == 0
        assert k0.sum() == 500 and part[n - 1, k0].sum() == (500 if everybody else 0)
        assert all(part[r, k0].any() for r in range(n - 1)) and not ((t[4][k0] >> (n - 1)) & 1).any()
        assert set(t[0][k0].tolist()) == set(range(n - 1))


def test_bit20_tick_reaches_above_2_to_the_20(oracle):
    t = S.bit20()
    m = len(t[0])
    assert m == (1 << 20) + 2052 and m % 4 == 0 and t[5].max() == m - 1 > (1 << 20)
    assert S.key_sizes(t, 2048).max() <= S.LIMITS[5]["kp_tc"] and S.bucket_width(5, m) == 2048
    for r in range(5):
        assert (np.sort(t[5][r]) == np.arange(m)).all()
        per = np.bincount((t[5][r].astype(np.int64) >> 11) * 2048 + t[2], minlength=1024 * 2048)
        assert per.max() <= 2                                       # words of one key in one bucket
    assert (t[5][4] >= (1 << 20)).sum() == 2052 and (t[5][2] >= (1 << 20)).sum() == 2052
