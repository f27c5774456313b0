"""Multi-key get / set commands, CPU side: tests/epaxos_multikey_sets.py (key tuples, explicit sets) reproduces the
reference's own k = 1 vectors (tests/golden/topone_multikey_k1.json, TopKConflictIndexTest.scala:280-330) and, with one
key per command, oracle/epaxos_sets.py."""
import json
import os

import numpy as np
import pytest

from oracle import epaxos_sets as single
from tests import epaxos_multikey_sets as mk
from tests.workloads import random_tick

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topone_multikey_k1.json")


def load_golden():
    g = json.load(open(GOLDEN))
    K = g["keys"]
    puts = [(tuple(p["instance"]), tuple(K[k] for k in p["keys"]), p["op"] == "set") for p in g["puts"]]
    queries = [(tuple(K[k] for k in q["keys"]), q["op"] == "set", q["top_one"]) for q in g["queries"]]
    return g, puts, queries


def test_model_reproduces_the_reference_k1_vectors():
    g, puts, queries = load_golden()
    rep = mk.Replica(0, g["num_leaders"], len(g["keys"]))
    for inst, keys, is_set in puts:
        rep.index_put(keys, is_set, inst)
    for keys, is_set, top in queries:
        assert rep.top_one_conflicts(keys, is_set) == top, (keys, is_set)


def test_model_rules_zero_keys_and_repeats():
    rep = mk.Replica(0, 3, 4)
    rep.index_put((1, 1, 2), True, (2, 5))
    assert rep.sets[1] == [0, 0, 6] and rep.sets[2] == [0, 0, 6]
    rep.index_put((), True, (0, 9))                                  # zero keys: put adds nothing
    assert all(v == 0 for row in rep.gets + [rep.sets[0], rep.sets[3]] for v in row)
    assert rep.top_one_conflicts((), True) == [0, 0, 0]              # ... and merges nothing
    assert rep.top_one_conflicts((1, 1), False) == rep.top_one_conflicts((1,), False)
    assert rep.compute_dependencies((0, 0), (), True) == set()


@pytest.mark.parametrize("n,fifo", [(3, True), (5, False), (7, True)])
def test_one_key_per_command_is_the_single_key_model(n, fifo):
    rng = np.random.default_rng(n)
    nxt = [0] * n
    a, b = single.EPaxos(n, 8), mk.EPaxos(n, 8)
    for _ in range(2):
        leader, number, key, is_set, mask, rank = random_tick(rng, n, 8, 120, nxt, 6.0, fifo=fifo)
        ra = a.tick(leader, number, key, is_set, mask, rank)
        rb = b.tick(leader, number, [(int(k),) for k in key], is_set, mask, rank)
        assert ra == rb
    for r in range(n):
        assert a.replicas[r].gets == b.replicas[r].gets and a.replicas[r].sets == b.replicas[r].sets
