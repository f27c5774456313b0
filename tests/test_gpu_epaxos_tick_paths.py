"""The EPaxos pre-accept tick (K5) at every table limit, with the proof that each tick took the path it was built for: the
ticks of tests/epaxos_tick_shapes.py run on the GPU, every output and every conflict index is compared with
oracle.EPaxos, and the WHOLE census of the context (include/fpx.h, fpx_epx_tick_census) is asserted by equality -- the
ticks are deterministic, so is the path of every key.  The four-array form and the packed form alternate.

Why no tick takes a radix sort of ONE pass, and none of TWO passes at n <= 5.  A key is radix-sorted only when a rank
bucket holds more than KP_MAX_OCC = 24 of one replica's words, and a bucket holds at most as many words as it is ranks
wide: 2^sh with sh = bits(m - 1) - log2(NBK).  A width above 24 is a width of 32 at least, so bits(m - 1) >= 5 + log2(NBK):
m > 16384 with NBK = 1024 (n = 3, 5), m > 8192 with NBK = 512 (n = 7).  The radix sort takes ceil(bits(m) / 7) passes: 3
from m = 16384 on, 2 from m = 128 on.  So one pass (m < 128) never meets a bucket wider than 1 rank, two passes
(m <= 16383) meet wide buckets only at n = 7 with 8193 <= m <= 16383; the second attempt's buckets over the key's own rank
range are never wider than the first's.  tests/test_epaxos_tick_shapes_cpu.py enumerates the widths; the census word of
the one-pass sort is asserted to be 0 in every case here, and that of the two-pass sort wherever n <= 5."""
import numpy as np
import pytest

from tests import epaxos_tick_shapes as S

pytestmark = pytest.mark.gpu
NS = [3, 5, 7]
ZERO = dict.fromkeys(("kp", "kp_handed_over", "v1_switched_off", "v1_keys", "v1_full", "v1_log_n3", "v1_index_bits",
                      "no_key_kernel", "scalar_loads", "sort_bucket1", "sort_bucket2", "sort_radix1", "sort_radix2",
                      "sort_radix3", "long_way"), 0)


def census_is(gpu, **words):
    assert gpu.tick_census() == dict(ZERO, **words)


def same_index(gpu, ref, n, num_keys):
    for r in range(n):
        for k in range(num_keys):
            a, b = gpu.read_index(r, k), ref.read_index(r, k)
            assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), (r, k)


def run(gpu, ref, tick, packed, triple_id=None):
    """one tick on both, every output compared: through fpx_epx_preaccept (host arrays in, the four arrays out) or through
    fpx_epx_preaccept_packed_dev (device arrays in, packed lines out)"""
    a, kw = S.args(tick)
    want = ref.preaccept(*a, triple_id=triple_id, **kw)
    assert want[0] == 0
    if not packed:
        got = gpu.preaccept(*a, triple_id=triple_id, **kw)
        assert got[0] == 0
        for x, y in zip(got[1:], want[1:]):
            np.testing.assert_array_equal(x, y)
        return
    import torch

    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]
    seen = torch.from_numpy(tick[6]).to(dev)
    tr = None if triple_id is None else torch.from_numpy(triple_id).to(dev)
    lines = torch.full((len(tick[0]), gpu.packed_stride()), -7, dtype=torch.int32, device=dev)
    gpu.preaccept_packed_dev(*t, lines, seen_mask=seen, triple_id=tr)
    assert gpu.sync() == 0
    fast, deps, ldeps, own = (x.cpu().numpy() for x in gpu.unpack(lines))
    np.testing.assert_array_equal(fast, want[1].astype(np.int32))
    np.testing.assert_array_equal(deps, want[2])
    np.testing.assert_array_equal(ldeps, want[3])
    np.testing.assert_array_equal(own, want[4])
    assert not lines[:, 2 * gpu.n + 3:].any()


def pair(oracle, n, num_keys, num_instances=0):
    from frankenpaxos_amd.epaxos import EPaxos

    return EPaxos(n, num_keys, num_instances=num_instances), oracle.EPaxos(n, num_keys, num_instances)


@pytest.mark.parametrize("n", NS)
def test_the_builders_limits_are_the_kernels(n):
    from frankenpaxos_amd.epaxos import EPaxos

    gpu = EPaxos(n, 4)
    assert gpu.limits() == S.LIMITS[n]
    census_is(gpu)


# ---------------------------------------------------------------------------------------------------- dispatch limits
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("num_keys", [2048, 2049])
def test_2048_keys_stay_in_the_second_form_and_2049_do_not(oracle, n, num_keys):
    m = 5000
    gpu, ref = pair(oracle, n, num_keys)
    assert num_keys - gpu.limits()["kp_maxb"] == (0 if num_keys == 2048 else 1)
    tick = S.assemble(n, (np.arange(m) * 37) % num_keys, S.rank_rows("reversed", n, m))
    run(gpu, ref, tick, packed=n == 5)
    same_index(gpu, ref, n, num_keys)
    if num_keys == 2048:
        census_is(gpu, kp=1, sort_bucket1=2048)      # (a bucket is 8 or 16 ranks wide)
    else:
        census_is(gpu, v1_keys=1)


@pytest.mark.parametrize("n", NS)
def test_one_key_exactly_full_and_one_command_more(oracle, n):
    gpu, ref = pair(oracle, n, 1)
    tc = gpu.limits()["kp_tc"]
    run(gpu, ref, S.sizes(n, [tc], kind="uniform"), packed=False)
    same_index(gpu, ref, n, 1)
    census_is(gpu, kp=1, sort_bucket1=1)
    gpu, ref = pair(oracle, n, 1)
    run(gpu, ref, S.sizes(n, [tc + 1], kind="uniform"), packed=True)
    same_index(gpu, ref, n, 1)
    # by dispatch, no partition launch; the first form holds 2048 commands of a key on chip at n = 3, fewer than tc + 1 else
    census_is(gpu, v1_full=1, long_way=0 if n == 3 else 1)


@pytest.mark.parametrize("n", NS)
def test_two_keys_full_then_overflowing_then_small(oracle, n):
    gpu, ref = pair(oracle, n, 2)
    tc = gpu.limits()["kp_tc"]
    nxt = [0] * n
    run(gpu, ref, S.sizes(n, [tc, 1], next_number=nxt), packed=True)
    census_is(gpu, kp=1, sort_bucket1=2, scalar_loads=1)                   # (tc + 1 commands: m % 4 != 0)
    run(gpu, ref, S.sizes(n, [tc + 1, 0], kind="reversed", next_number=nxt), packed=False)
    census_is(gpu, kp=1, kp_handed_over=1, sort_bucket1=2, scalar_loads=2, long_way=0 if n == 3 else 1)
    # the claim counters were left at zero by the tick that was handed over: a small tick is partitioned correctly
    run(gpu, ref, S.sizes(n, [6, 6], seed=2, next_number=nxt), packed=True)
    census_is(gpu, kp=2, kp_handed_over=1, sort_bucket1=4, scalar_loads=2, long_way=0 if n == 3 else 1)
    same_index(gpu, ref, n, 2)


@pytest.mark.parametrize("n", NS)
def test_the_command_log_takes_the_first_form_at_three_replicas_only(oracle, n):
    from frankenpaxos_amd.epaxos import EPaxos

    tc = EPaxos(n, 3).limits()["kp_tc"]
    tick = S.sizes(n, [tc, 200, 100], kind="reversed")
    m = len(tick[0])
    gpu, ref = pair(oracle, n, 3, num_instances=m)
    tr = ((np.arange(m) * 7919) % (1 << 20)).astype(np.int32)
    run(gpu, ref, tick, packed=n == 7, triple_id=tr)
    same_index(gpu, ref, n, 3)
    for r in range(n):
        for i in range(r, m, 37):
            L, x = int(tick[0][i]), int(tick[1][i])
            assert gpu.read_cmdlog(r, L, x) == ref.read_cmdlog(r, L, x)
            a, b = gpu.read_cmdlog_deps(r, L, x), ref.read_cmdlog_deps(r, L, x)
            assert a[0].tolist() == b[0].tolist() and a[1] == b[1]
    if n == 3:
        census_is(gpu, v1_log_n3=1)
    else:
        census_is(gpu, kp=1, sort_bucket1=3)


# -------------------------------------------------------------------------------------------------------- sort routes
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("members", [24, 25])
def test_a_bucket_of_24_words_is_sorted_in_place_and_one_of_25_is_not(oracle, n, members):
    gpu, ref = pair(oracle, n, 40)
    run(gpu, ref, S.one_bucket(n, 20000, members), packed=members == 25)
    same_index(gpu, ref, n, 40)
    if members == 24:
        census_is(gpu, kp=1, sort_bucket1=40)
    else:
        census_is(gpu, kp=1, sort_bucket1=39, sort_bucket2=1)   # 25 neighbours: one word per bucket of the key's own range


@pytest.mark.parametrize("n", NS)
def test_clumps_at_both_ends_take_three_radix_passes(oracle, n):
    gpu, ref = pair(oracle, n, 40)
    run(gpu, ref, S.clumps(n, 20000), packed=n == 3)
    same_index(gpu, ref, n, 40)
    census_is(gpu, kp=1, sort_bucket1=39, sort_radix3=1)


def test_clumps_in_a_tick_of_12000_take_two_radix_passes_at_seven_replicas(oracle):
    gpu, ref = pair(oracle, 7, 40)
    run(gpu, ref, S.clumps(7, 12000), packed=False)
    same_index(gpu, ref, 7, 40)
    census_is(gpu, kp=1, sort_bucket1=39, sort_radix2=1)


# ----------------------------------------------------------------------------------------------------- bucket details
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("members", [4, 5])
def test_buckets_of_four_and_of_five_members(oracle, n, members):
    """four members are read by the unrolled loads alone, the fifth by the loop behind them: 40 such buckets each"""
    gpu, ref = pair(oracle, n, 80)
    run(gpu, ref, S.many_small_buckets(n, 20480, members), packed=members == 4)
    same_index(gpu, ref, n, 80)
    census_is(gpu, kp=1, sort_bucket1=80)


@pytest.mark.parametrize("n", NS)
def test_the_last_bucket_of_either_attempt(oracle, n):
    gpu, ref = pair(oracle, n, 40)
    run(gpu, ref, S.last_bucket(n), packed=False)
    same_index(gpu, ref, n, 40)
    census_is(gpu, kp=1, sort_bucket1=40)
    gpu, ref = pair(oracle, n, 40)
    run(gpu, ref, S.last_bucket_second_attempt(n), packed=True)
    same_index(gpu, ref, n, 40)
    census_is(gpu, kp=1, sort_bucket1=39, sort_bucket2=1)


# ---------------------------------------------------------------------------------------------------------- key sizes
@pytest.mark.parametrize("n", NS)
def test_keys_of_every_size_class_in_one_tick(oracle, n):
    counts = S.key_size_counts(n)
    gpu, ref = pair(oracle, n, len(counts))
    nxt = [0] * n
    run(gpu, ref, S.sizes(n, counts, next_number=nxt), packed=False)
    census_is(gpu, kp=1, sort_bucket1=9)                       # nine keys have commands; no bucket is wider than 8 ranks
    run(gpu, ref, S.sizes(n, counts, seed=1, kind="reversed", everybody=True, next_number=nxt), packed=True)
    census_is(gpu, kp=2, sort_bucket1=18)
    same_index(gpu, ref, n, len(counts))


@pytest.mark.parametrize("n", NS)
def test_ticks_of_one_two_and_five_commands_among_2048_keys(oracle, n):
    gpu, ref = pair(oracle, n, 2048)
    nxt = [0] * n
    for j, keys in enumerate(([2047], [0, 2047], [5, 5, 6, 2047, 0])):
        tick = S.assemble(n, np.array(keys), S.rank_rows("reversed", n, len(keys)), next_number=nxt)
        run(gpu, ref, tick, packed=j == 1)
    same_index(gpu, ref, n, 2048)
    census_is(gpu, kp=3, scalar_loads=3, sort_bucket1=1 + 2 + 4)


# ------------------------------------------------------------------------------------------------------ participation
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("everybody", [False, True])
def test_a_replica_that_takes_part_in_none_of_a_keys_commands(oracle, n, everybody):
    gpu, ref = pair(oracle, n, 6)
    run(gpu, ref, S.absent_replica(n, everybody=everybody), packed=everybody)
    same_index(gpu, ref, n, 6)
    census_is(gpu, kp=1, sort_bucket1=6)


# -------------------------------------------------------------------------------------------------------- rank shapes
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["uniform", "reversed"])
def test_uniform_permutations_and_a_reversed_replica_over_two_ticks(oracle, n, kind):
    num_keys, m = 16, 6000
    gpu, ref = pair(oracle, n, num_keys)
    nxt = [0] * n
    for tick in range(2):
        key = (np.arange(m) * (5 + 6 * tick)) % num_keys
        t = S.assemble(n, key, S.rank_rows(kind, n, m, seed=10 * n + tick), everybody=tick == 1, next_number=nxt)
        run(gpu, ref, t, packed=tick == 0)
    same_index(gpu, ref, n, num_keys)
    census_is(gpu, kp=2, sort_bucket1=32)                      # a bucket is 8 or 16 ranks wide


# ----------------------------------------------------------------------------------------------------- the first form
@pytest.mark.parametrize("n", NS)
def test_the_first_forms_own_table_limit(oracle, monkeypatch, n):
    """FPX_EPX_V1: k_epx_key holds KeyTile<N>::TC commands of a key; the key with one more goes the long way.  The same
    tick on a second-form context: the same answers (there the key overflows the second form's tables at n = 3 and 5)"""
    from frankenpaxos_amd.epaxos import EPaxos

    monkeypatch.setenv("FPX_EPX_V1", "1")
    v1 = EPaxos(n, 3)
    monkeypatch.delenv("FPX_EPX_V1")
    tc = v1.limits()["key_tc"]
    tick = S.sizes(n, [tc, tc + 1, 50], kind="uniform", seed=n)
    ref = oracle.EPaxos(n, 3)
    run(v1, ref, tick, packed=False)
    same_index(v1, ref, n, 3)
    census_is(v1, v1_switched_off=1, long_way=1)
    v2, ref = EPaxos(n, 3), oracle.EPaxos(n, 3)
    run(v2, ref, tick, packed=True)
    same_index(v2, ref, n, 3)
    if n == 7:      # 577 commands fit the second form's 640
        census_is(v2, kp=1, scalar_loads=1, sort_bucket1=3)
    else:
        census_is(v2, kp_handed_over=1, scalar_loads=1, long_way=1)


# ------------------------------------------------------------------------------------------------------------- bit 20
def test_ranks_and_indices_above_2_to_the_20(oracle):
    """the one large tick: 2^20 + 2052 commands of 2048 keys at n = 5 through partition, records (bit 20 of the index and of
    every rank, the split rank included), sort and decision"""
    gpu, ref = pair(oracle, 5, 2048)
    tick = S.bit20()
    assert tick[5].max() > (1 << 20)
    run(gpu, ref, tick, packed=True)
    same_index(gpu, ref, 5, 2048)
    census_is(gpu, kp=1, sort_bucket1=2048)
