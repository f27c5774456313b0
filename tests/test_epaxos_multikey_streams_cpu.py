"""The reference of tests/test_gpu_epaxos_multikey_handlers.py, checked without a GPU.

1. The batch drivers of tests/epaxos_multikey_streams.py (the set model, one message at a time) equal the C oracle's
   BATCH calls on random one-key streams: every reply bit, nack_ballot, the decoded reply dependencies, committed,
   status 0 / 9, and the final command logs, indices and largestBallot.  That is what licenses the drivers as the
   reference for real key lists, where no second restatement exists.
2. The multi-key streams the GPU tests replay reach what they claim -- judged from the model's answers alone."""
import pytest

from tests import epaxos_multikey_sets as mk
from tests import epaxos_multikey_streams as S
from tests.epaxos_multikey_streams import MULTIKEY_SHAPES, SEED, STEPS


@pytest.mark.parametrize("n,NI,m,num_keys", [(3, 64, 40, 4), (5, 512, 700, 8), (7, 300, 1500, 3)])
def test_batch_drivers_equal_the_c_oracle_on_one_key_streams(oracle, n, NI, m, num_keys):
    ref, model = oracle.EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    ops = S.multikey_stream(900 + n, n, NI, m, num_keys, max_keys=None, steps=16 if m < 100 else 8)
    results = []
    for op in ops:
        want = S.apply_model(model, op, noop_is_none=True)
        S.assert_same(op, S.decoded(op, S.apply_single_key(ref, op)), want)
        results.append(want)
    c = S.coverage(n, ops, results)
    assert c["ok"] and c["nack"] and c["commit"] and c["fatal"] and c["committed"], c
    every = [(L, x) for L in range(n) for x in range(NI)]
    S.compare_state(ref, model, n, NI, num_keys, every)


@pytest.mark.parametrize("n,NI,m,num_keys", MULTIKEY_SHAPES)
def test_multikey_streams_reach_what_they_claim(n, NI, m, num_keys):
    model = mk.EPaxos(n, num_keys)
    ops = S.multikey_stream(SEED + n, n, NI, m, num_keys, max_keys=8, steps=STEPS[n])
    assert [k for k, _ in ops].count("hp") >= 2 and {k for k, _ in ops} == {"tick", "hp", "accept", "prepare", "commit"}
    assert any(a["deps"] is None for k, a in ops if k == "commit") or n == 7       # (n = 7 stops before the Commits by id)
    c = S.coverage(n, ops, [S.apply_model(model, op) for op in ops])
    assert c["ok"] and c["nack"] and c["zero_keys"] and c["repeated_key"] and c["one_distinct"] and c["split_pair"], c
    if m > 40:
        counts = ("ok", "resend", "nack", "commit", "ignored", "fatal", "committed")
        assert all(c[k] > 0 for k in counts), c
        # m > CL_TILE = 1024 messages, P > RS_TILE = 4096 pairs, P % 4 != 0, and a Nack outside the first Nack tile
        assert c["big_batch"] and c["big_batch_late_nack"], c


def test_an_empty_key_list_and_a_noop_are_one_command_to_the_model():
    n, NI, num_keys = 5, 64, 4
    a, b = mk.EPaxos(n, num_keys), mk.EPaxos(n, num_keys)
    ops = S.multikey_stream(7, n, NI, 60, num_keys, max_keys=None, steps=8)
    assert any(len(ks) == 0 for _, o in ops for ks in o.get("keys") or ())
    for op in ops:
        assert S.apply_model(a, op, noop_is_none=True) == S.apply_model(b, op)
    for ra, rb in zip(a.replicas, b.replicas):
        assert ra.gets == rb.gets and ra.sets == rb.sets and ra.largest_ballot == rb.largest_ballot
        assert {k: vars(v) for k, v in ra.cmd_log.items()} == {k: vars(v) for k, v in rb.cmd_log.items()}
