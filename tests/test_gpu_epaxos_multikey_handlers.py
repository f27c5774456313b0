"""The multi-key message handlers (fpx_epx_handle_preaccept_mk, fpx_epx_accept_mk, fpx_epx_handle_commit_mk) on whole
batches: more than one workgroup, sort tile (RS_TILE = 4096 pairs) and Nack tile (CL_TILE = 1024 messages), messages of
one batch that conflict through a shared key at one replica and not at another, replicas that Nack / resend / ignore part
of a batch, batches with fewer pairs than messages and with none.

  a. one-key lists through the _mk entry points against the C oracle's single-key calls: exact, up to m = 5000
  b. the two-pass key sort (num_keys >= 2048) under K7 in both forms
  c. real key lists against the set model's batch drivers (tests/epaxos_multikey_streams.py; licensed as a reference
     and examined for what they reach by tests/test_epaxos_multikey_streams_cpu.py), and small cases of their own
  d. handle_commit_mk at size against the C oracle fed one single-key Commit per distinct key"""
import time

import numpy as np
import pytest

from tests import epaxos_multikey_sets as mk
from tests import epaxos_multikey_streams as S
from tests.test_epaxos import _cl_batch, _same
from tests.workloads import random_tick

pytestmark = pytest.mark.gpu


def same_state(gpu, ref, n, NI, num_keys, instances, keys=None):
    """command log, stored dependencies and conflict indices, arrays as they are: device == C oracle"""
    for r in range(n):
        for L, x in instances:
            assert gpu.read_cmdlog(r, L, x) == ref.read_cmdlog(r, L, x), (r, L, x)
            (da, ea), (db, eb) = gpu.read_cmdlog_deps(r, L, x), ref.read_cmdlog_deps(r, L, x)
            assert ea == eb and da.tolist() == db.tolist(), (r, L, x)
        for k in range(num_keys) if keys is None else keys:
            for a, b in zip(gpu.read_index(r, k), ref.read_index(r, k)):
                np.testing.assert_array_equal(a, b)


def reply_counts(ops, outs):
    c = dict(ok=0, resend=0, nack=0, commit=0, ignored=0, fatal=0, committed=0)
    for (kind, a), out in zip(ops, outs):
        if kind == "hp":
            st, ok, resend, nack, com = out[:5]
            for name, bits in (("ok", ok), ("resend", resend), ("nack", nack), ("commit", com)):
                c[name] += int(np.unpackbits(bits).sum())
            c["ignored"] += int(np.unpackbits(a["tgt"] & ~(ok | resend | nack | com)).sum())
        elif kind == "accept":
            c["fatal"] += out[0] != 0
            c["committed"] += int(out[5].sum())
    return c


# ---- a. one key per command: the pair pipeline must be the single-key handler, bit for bit ----------------------------
@pytest.mark.parametrize("n,NI,m,num_keys", [(3, 64, 40, 4), (5, 512, 700, 8), (7, 300, 1500, 3), (5, 4096, 5000, 64)])
def test_one_key_lists_through_the_mk_entry_points_equal_the_c_oracle(oracle, n, NI, m, num_keys):
    """the streams of the single-key K6 / K7 / handleCommit tests in one rotation (ticks, PreAccepts in random ballots and
    the old leaders' own, Accepts sent and re-sent, Prepares, Commits with and without dependencies), every command as a
    list of one key, a Noop as the empty list: every output array of every call, then command log, stored dependencies
    and every index row, device _mk == C oracle single-key"""
    from frankenpaxos_amd.epaxos import EPaxos

    gpu, ref = EPaxos(n, num_keys, num_instances=NI), oracle.EPaxos(n, num_keys, num_instances=NI)
    ops = S.multikey_stream(300 + n + NI, n, NI, m, num_keys, max_keys=None, steps=16)
    outs = []
    for op in ops:
        a, b = S.apply_multikey(gpu, op), S.apply_single_key(ref, op)
        _same(a, b)
        outs.append(a)
    c = reply_counts(ops, outs)
    print(c)
    assert c["ok"] > 0 and c["nack"] > 0 and (m < 500 or all(v > 0 for v in c.values())), c
    if m >= 5000:
        assert max(len(a["leader"]) for k, a in ops if k == "hp") == 5000
    rng = np.random.default_rng(n)
    same_state(gpu, ref, n, NI, num_keys, S.sampled_instances(rng, n, NI, 300) + S.instances_of(ops[-1])[:300])
    gpu.close()


# ---- b. num_keys >= 2048: sort_by_key takes two passes, launch_segments finds the segments without the key totals ------
@pytest.mark.parametrize("num_keys", [2047, 2048])
def test_k7_on_both_sides_of_the_two_pass_key_sort(oracle, num_keys):
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI, m = 5, 512, 700
    single, multi = EPaxos(n, num_keys, num_instances=NI), EPaxos(n, num_keys, num_instances=NI)
    ref = oracle.EPaxos(n, num_keys, num_instances=NI)
    ops = S.multikey_stream(2048, n, NI, m, num_keys, max_keys=None, steps=8)
    # few distinct keys among many: messages of one batch still meet on a key (keys at both ends of the range included)
    hot = np.r_[0, 1, num_keys - 2, num_keys - 1, np.random.default_rng(1).integers(0, num_keys, 12)].astype(np.int32)
    for a in {id(a): a for _, a in ops}.values():                      # (an Accept step is one dict, twice)
        if "key" in a:
            a["key"] = np.where(a["key"] >= 0, hot[a["key"] % len(hot)], -1).astype(np.int32)
            a["keys"] = S.lists_of(a["key"])
    outs = []
    for op in ops:
        want = S.apply_single_key(ref, op)
        _same(S.apply_single_key(single, op), want)
        _same(S.apply_multikey(multi, op), want)
        outs.append(want)
    c = reply_counts(ops, outs)
    assert c["ok"] > 0 and c["nack"] > 0 and c["resend"] > 0, c
    inst = S.sampled_instances(np.random.default_rng(2), n, NI, 200)
    for gpu in (single, multi):
        same_state(gpu, ref, n, NI, num_keys, inst, keys=sorted(set(hot.tolist())) + [2, num_keys // 2])
        gpu.close()


# ---- c. real key lists against the set model ---------------------------------------------------------------------------
def replay(gpu, model, ops, n, NI, num_keys, seed=0):
    """every reply of every batch against the model's batch drivers, and the state after each batch: over all instances
    at NI = 64, over 300 sampled instances plus every instance of the batch otherwise"""
    rng = np.random.default_rng(seed)
    t = dict(model=0.0, device=0.0, decode=0.0, state=0.0)
    for op in ops:
        t0 = time.perf_counter()
        want = S.apply_model(model, op)
        t1 = time.perf_counter()
        out = S.apply_multikey(gpu, op)
        t2 = time.perf_counter()
        S.assert_same(op, S.decoded(op, out), want)
        t3 = time.perf_counter()
        every = [(L, x) for L in range(n) for x in range(NI)]
        S.compare_state(gpu, model, n, NI, num_keys,
                        every if NI <= 64 else S.sampled_instances(rng, n, NI, 300) + S.instances_of(op))
        t4 = time.perf_counter()
        for k, d in zip(("model", "device", "decode", "state"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[k] += d
    print("seconds:", {k: round(v, 2) for k, v in t.items()})


@pytest.mark.parametrize("n,NI,m,num_keys", S.MULTIKEY_SHAPES)
def test_key_list_batches_match_the_set_model(n, NI, m, num_keys):
    """lists of 0 .. 8 keys with repeats over few keys, so that the messages of a batch collide: the rotation of
    tests/epaxos_multikey_streams.py (at the two larger shapes a PreAccept batch has m > 1024 messages and P > 4096 pairs)"""
    from frankenpaxos_amd.epaxos import EPaxos

    gpu, model = EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    ops = S.multikey_stream(S.SEED + n, n, NI, m, num_keys, max_keys=8, steps=S.STEPS[n])
    replay(gpu, model, ops, n, NI, num_keys, seed=n)
    gpu.close()


def test_a_batch_of_empty_key_lists_is_a_batch_of_noops():
    """P = 0 with m = 300 between two ordinary batches: the replies the model gives, the replies the single-key form
    gives for Noops (key -1) on a second context with the same history, and no index row moves"""
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI, num_keys = 5, 128, 8
    rng = np.random.default_rng(30)
    nxt = [NI // 2] * n                                                  # no tick follows: every number may be drawn
    before, empty, after = (S.hp_op(rng, n, NI, 300, num_keys, nxt, keys=k) for k in (None, lambda mm: [[] for _ in range(mm)], None))
    gpu, twin, model = EPaxos(n, num_keys, num_instances=NI), EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    replay(gpu, model, [before], n, NI, num_keys)
    S.apply_multikey(twin, before)
    index = [[a.tolist() for a in gpu.read_index(r, k)] for r in range(n) for k in range(num_keys)]
    assert any(any(row) for pair in index for row in pair)
    a = empty[1]
    assert len(a["leader"]) == 300 and sum(len(ks) for ks in a["keys"]) == 0
    want = S.apply_model(model, empty)
    out = S.apply_multikey(gpu, empty)
    S.assert_same(empty, S.decoded(empty, out), want)
    assert sum(want[1]) > 0 and sum(want[3]) > 0                           # some processed, some Nacked
    _same(out, twin.handle_preaccept(a["leader"], a["number"], a["b_ord"], a["b_rep"], np.full(300, -1, np.int32), a["is_set"],
                                     a["triple"], a["din"], a["dend"], a["tgt"]))
    assert index == [[x.tolist() for x in gpu.read_index(r, k)] for r in range(n) for k in range(num_keys)]
    S.compare_state(gpu, model, n, NI, num_keys, S.instances_of(empty))
    replay(gpu, model, [after], n, NI, num_keys)
    for e in (gpu, twin):
        e.close()


def test_one_command_with_forty_keys_drawn_from_three():
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI, num_keys = 5, 64, 3
    rng = np.random.default_rng(31)
    nxt = [0] * n
    long_list = rng.integers(0, num_keys, 40).tolist()
    assert len(set(long_list)) == 3
    ops = [S.hp_op(rng, n, NI, 60, num_keys, nxt), S.hp_op(rng, n, NI, 1, num_keys, nxt, keys=lambda mm: [long_list]),
           S.hp_op(rng, n, NI, 60, num_keys, nxt)]
    ops[1][1]["tgt"][:] = 0b10111
    gpu, model = EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    replay(gpu, model, ops, n, NI, num_keys)
    gpu.close()


@pytest.mark.parametrize("n,NI,m", [(3, 86, 257), (5, 206, 1025)])
def test_one_message_past_a_workgroup_and_past_a_nack_tile(n, NI, m):
    """m = 257 (one message in the second workgroup of the per-message kernels) and m = 1025 (one message in the second
    Nack tile), both 1 mod 4 (the reply bits are OR-ed into 32-bit words of four messages): three batches over nearly
    every instance of a small command log (small, so that the model's sets stay small), so that the later batches are
    Nacked, answered again and processed in higher ballots"""
    from frankenpaxos_amd.epaxos import EPaxos

    num_keys = 8
    rng = np.random.default_rng(m)
    used = [NI // 2] * n                                                 # no tick follows: every number may be drawn
    ops = [S.hp_op(rng, n, NI, m, num_keys, used) for _ in range(3)]
    assert all(len(a["leader"]) == m for _, a in ops) and n * NI - m < 8
    ops[2][1]["b_ord"][-1], ops[2][1]["tgt"][-1] = 0, (1 << n) - 1       # the last message meets what it can of Nacks
    gpu, model = EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    replay(gpu, model, ops, n, NI, num_keys)
    assert model.replicas[0].cmd_log[S.instances_of(ops[2])[-1]].kind in (2, 3, 4)
    gpu.close()


@pytest.mark.parametrize("tick_first", [True, False])
def test_pair_scratch_is_reused_at_a_smaller_size(tick_first):
    """mk_pair / mk_pconf / kv are sized by the largest call so far: a PreAccept batch after a larger pre-accept tick,
    and a tick after a larger PreAccept batch, must not read what the larger call left behind"""
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI, num_keys = 5, 512, 8
    rng = np.random.default_rng(40 + tick_first)
    nxt = [0] * n
    if tick_first:
        ops = [S.tick_op(rng, n, 600, num_keys, nxt), S.hp_op(rng, n, NI, 100, num_keys, nxt)]
    else:
        ops = [S.hp_op(rng, n, NI, 700, num_keys, nxt), S.tick_op(rng, n, 60, num_keys, nxt), S.hp_op(rng, n, NI, 90, num_keys, nxt)]
    gpu, model = EPaxos(n, num_keys, num_instances=NI), mk.EPaxos(n, num_keys)
    replay(gpu, model, ops, n, NI, num_keys)
    gpu.close()


# ---- d. handle_commit_mk at size: a Commit with keys K leaves what one single-key Commit per distinct key leaves ---------
def test_handle_commit_mk_at_size_equals_one_single_key_commit_per_distinct_key(oracle):
    """(5, 4096, 5000) with 0 .. 8 keys per Commit, after a tick and an Accept batch (instances in every state), with
    dependencies and by triple id alone: the C oracle takes the expanded batch -- message i once per distinct key, the
    same triple, dependencies and recipients (include/fpx.h allows repeats with the same triple), key -1 for no keys"""
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI, m, num_keys = 5, 4096, 5000, 64
    gpu, ref = EPaxos(n, num_keys, num_instances=NI), oracle.EPaxos(n, num_keys, num_instances=NI)
    rng = np.random.default_rng(50)
    nxt = [0] * n
    tick = random_tick(rng, n, num_keys, 400, nxt, 3.0)
    tr = rng.integers(0, 1 << 20, 400).astype(np.int32)
    _same(gpu.preaccept(*tick, triple_id=tr), ref.preaccept(*tick, triple_id=tr))
    leader, number, b_ord, b_rep, tgt = _cl_batch(rng, n, NI, m, nxt)
    tgt = (tgt & ~(1 << b_rep)).astype(np.uint8)
    tr = rng.integers(0, 1 << 20, m).astype(np.int32)
    _same(gpu.accept(leader, number, b_ord, b_rep, tr, tgt), ref.accept(leader, number, b_ord, b_rep, tr, tgt))
    last = None
    for by_id in (False, True):
        leader, number, _, _, tgt = _cl_batch(rng, n, NI, m, nxt)
        assert len(leader) == m
        keys = S.random_key_lists(rng, m, num_keys, 8)
        is_set = (rng.random(m) < 0.5).astype(np.uint8)
        tr = rng.integers(0, 1 << 20, m).astype(np.int32)
        deps, ends = (None, None) if by_id else S._deps(rng, NI, n, leader, number)
        assert gpu.handle_commit_mk(leader, number, tr, tgt, keys, is_set, deps=deps, deps_values_end=ends) == 0
        distinct = [sorted(set(ks)) or [-1] for ks in keys]
        idx = np.repeat(np.arange(m), [len(d) for d in distinct])
        key = np.array([k for d in distinct for k in d], np.int32)
        assert len(idx) > 3 * m
        assert ref.handle_commit(leader[idx], number[idx], tr[idx], tgt[idx], key=key, is_set=is_set[idx],
                                 deps=None if by_id else deps[idx], deps_values_end=None if by_id else ends[idx]) == 0
        last = [(int(L), int(x)) for L, x in zip(leader[:300], number[:300])]
    same_state(gpu, ref, n, NI, num_keys, S.sampled_instances(rng, n, NI, 300) + last)
    gpu.close()
