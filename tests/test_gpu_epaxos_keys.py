"""The device key table (fpx_epx_keys_*, csrc/fpx_intern.hpp) against a Python dict filled in first-occurrence order: the ids
must be EQUAL, not merely consistent.  Contexts have num_keys = 8 (16 slots) unless said, so every batch collides somewhere;
keys are chosen by the table's own hash (FNV-1a 64, tests/test_epaxos_cmd_parse_cpu.py holds it against the header) where a
test needs a particular chain."""
import random

import numpy as np
import pytest

from tests.epaxos_cmd_cases import KeyDict
from tests.test_epaxos_cmd_parse_cpu import fnv1a64

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = 1, 5


def ctx(num_keys=8, arena=1 << 16):
    from frankenpaxos_amd.epaxos import EPaxos

    e = EPaxos(3, num_keys)
    e.keys_enable(arena)
    return e


def same_as_dict(e, d, keys):
    st, ids = e.keys_intern(keys)
    assert st == 0
    assert ids.tolist() == d.intern(keys)
    order = d.order()
    assert e.keys_count() == (len(order), sum(len(k) for k in order))
    assert e.keys_read() == order


def keys_with_home(slot, count, slots=16, prefix=b"h"):
    out, j = [], 0
    while len(out) < count:
        k = prefix + b"%d" % j
        if fnv1a64(k) & (slots - 1) == slot:
            out.append(k)
        j += 1
    return out


def test_eight_distinct_keys_fill_the_table():
    e, d = ctx(), KeyDict()
    # four keys at home in slot 3 and four in slot 4, alternating: the two chains run through each other
    keys = [k for pair in zip(keys_with_home(3, 4, prefix=b"c"), keys_with_home(4, 4, prefix=b"d")) for k in pair]
    assert sorted({fnv1a64(k) & 15 for k in keys}) == [3, 4] and len(set(keys)) == 8
    same_as_dict(e, d, keys)
    same_as_dict(e, d, keys[::-1])                              # all resident now: the same ids, nothing new
    e.close()


def test_a_chain_of_eight_wraps_the_table_end():
    e, d = ctx(), KeyDict()
    keys = keys_with_home(15, 8)
    assert len(set(keys)) == 8
    same_as_dict(e, d, keys)
    same_as_dict(e, d, [keys[7], keys[0], keys[3]])
    e.close()


def test_600_strings_over_8_keys():
    """several workgroups and scan tiles; most repeats of a key sit in another workgroup than its first occurrence"""
    e, d = ctx(), KeyDict()
    rng = random.Random(6)
    keys = [b"key-%d" % j for j in range(8)]
    batch = [keys[j % 8] for j in range(600)]
    rng.shuffle(batch)
    first = {k: batch.index(k) for k in keys}
    assert sum(1 for j, k in enumerate(batch) if j // 256 != first[k] // 256) > 300
    same_as_dict(e, d, batch)
    e.close()


def test_three_batches_mix_resident_and_new_keys():
    e, d = ctx(), KeyDict()
    same_as_dict(e, d, [b"a", b"b", b"a", b"c"])
    same_as_dict(e, d, [b"d", b"a", b"e", b"d", b"c", b"f"])
    same_as_dict(e, d, [b"f", b"g", b"b", b"h", b"g"])
    assert e.keys_count()[0] == 8
    e.close()


def test_the_empty_key_and_two_long_keys_that_differ_in_the_last_byte():
    e, d = ctx(arena=3 * 4096), KeyDict()
    long_a = bytes(j % 251 for j in range(4096))
    long_b = long_a[:-1] + b"\x00"
    assert long_a != long_b
    same_as_dict(e, d, [b"", long_a, b"x", long_b, b"", long_a])
    same_as_dict(e, d, [long_b, b"", long_a])
    # one byte more than a key may have: refused at that string, nothing applied
    before = (e.keys_count(), e.keys_read())
    st, ids = e.keys_intern([b"y", long_a + b"z", b"w"])
    assert st == EINVAL and (ids == -9).all()
    assert (e.keys_count(), e.keys_read()) == before
    same_as_dict(e, d, [b"y", b"w"])
    e.close()


def test_the_ninth_key_is_refused_and_the_batch_rolled_back():
    e, d = ctx(), KeyDict()
    same_as_dict(e, d, [b"k%d" % j for j in range(5)])
    before = (e.keys_count(), e.keys_read())
    batch = [b"k2", b"n0", b"n1", b"k0", b"n2", b"n3", b"n1"]  # 5 + 4 distinct
    st, ids = e.keys_intern(batch)
    assert st == ECAPACITY and (ids == -9).all()
    assert (e.keys_count(), e.keys_read()) == before
    # the same batch minus the offender: were a pending slot left behind, n0 .. n2 would miss their ids or the table fill up
    same_as_dict(e, d, [k for k in batch if k != b"n3"])
    assert e.keys_count()[0] == 8
    st, ids = e.keys_intern([b"one more"])
    assert st == ECAPACITY
    same_as_dict(e, d, batch[:3])
    e.close()


def test_an_arena_one_byte_too_small():
    keys = [b"alpha", b"be", b"", b"gamma7"]
    need = sum(len(k) for k in keys)
    e, d = ctx(arena=need - 1), KeyDict()
    st, ids = e.keys_intern(keys)
    assert st == ECAPACITY and (ids == -9).all()
    assert e.keys_count() == (0, 0) and e.keys_read() == []
    same_as_dict(e, d, keys[:3] + [b"gamma"])                  # one byte less: it fits exactly
    assert e.keys_count() == (4, need - 1)
    e.close()
    e, d = ctx(arena=need), KeyDict()
    same_as_dict(e, d, keys)
    e.close()


def test_3000_distinct_keys_in_one_batch():
    e, d = ctx(num_keys=4096, arena=1 << 16), KeyDict()
    rng = random.Random(30)
    distinct = [b"%d" % rng.randrange(10 ** 9) for _ in range(3000)]
    distinct = list(dict.fromkeys(distinct))
    batch = distinct + [rng.choice(distinct) for _ in range(5000 - len(distinct))]
    rng.shuffle(batch)
    assert len(batch) == 5000
    same_as_dict(e, d, batch)
    assert e.keys_count()[0] == len(distinct)
    # part of the table, and a buffer that is too small for it
    assert e.keys_read(100, 50) == d.order()[100:150]
    off = np.zeros(11, np.int32)
    out = np.zeros(4, np.uint8)
    assert e.L.fpx_epx_keys_read(e._h, 0, 10, off.ctypes.data, out.ctypes.data, 4) == ECAPACITY
    assert off[10] == sum(len(k) for k in d.order()[:10])
    assert e.L.fpx_epx_keys_read(e._h, len(distinct) - 1, 2, off.ctypes.data, out.ctypes.data, 4) == EINVAL
    e.close()


def test_the_device_form_equals_the_host_form():
    import torch

    host, dev, d = ctx(), ctx(), KeyDict()
    rng = random.Random(9)
    pool = [b"p%d" % j for j in range(8)]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for size in (1, 7, 300):
        batch = [rng.choice(pool[:3 + size % 6]) for _ in range(size)]
        buf, off, ln = host.pack_keys(batch)
        st, want = host.keys_intern(batch)
        assert st == 0 and want.tolist() == d.intern(batch)
        ids = torch.full((size,), -9, dtype=torch.int32, device="cuda")
        dev.keys_intern_dev(T(buf), T(off), T(ln), ids)
        assert dev.sync() == 0
        np.testing.assert_array_equal(ids.cpu().numpy(), want)
    assert dev.keys_read() == host.keys_read() == d.order()
    # a refused device batch: ids of -1, the status through sync, the table as before
    batch = [b"q%d" % j for j in range(9)]
    buf, off, ln = host.pack_keys(batch)
    ids = torch.full((9,), -9, dtype=torch.int32, device="cuda")
    dev.keys_intern_dev(T(buf), T(off), T(ln), ids)
    assert dev.sync() == ECAPACITY
    assert (ids.cpu().numpy() == -1).all() and dev.keys_read() == d.order()
    # a string that leaves the buffer
    off2 = off.copy()
    off2[4] = len(buf) - 1
    dev.keys_intern_dev(T(buf), T(off2), T(ln), ids)
    assert dev.sync() == EINVAL and dev.keys_read() == d.order()
    host.close(), dev.close()


def test_the_table_is_opt_in():
    from frankenpaxos_amd.epaxos import EPaxos, FpxError

    e = EPaxos(3, 8)
    assert e.keys_intern([b"a"])[0] == EINVAL
    with pytest.raises(FpxError):
        e.keys_count()
    e.keys_enable(64)
    with pytest.raises(FpxError) as err:
        e.keys_enable(64)
    assert err.value.status == EINVAL
    assert e.keys_intern([])[0] == 0 and e.keys_count() == (0, 0)
    e.close()
