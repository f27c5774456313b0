"""A multi-key burst through the JNI natives the Scala actor calls (epxPreacceptMk, epxHandleCommitMk), run on the mock
JVM of tests/test_jni_shim.py, against tests/epaxos_multikey_sets.py."""
import ctypes as C

import numpy as np
import pytest

from tests import epaxos_multikey_sets as mk
from tests.test_epaxos_models import decode
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)
from tests.workloads import random_tick

pytestmark = pytest.mark.gpu


def test_multikey_burst_through_the_natives_equals_the_model(jvm):  # noqa: F811
    n, NK, NI, m = 5, 10, 512, 200
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    rng = np.random.default_rng(3)
    leader, number, _, is_set, mask, rank = random_tick(rng, n, NK, m, [0] * n, 5.0)
    lists = [list(rng.integers(0, NK, int(c))) for c in rng.integers(0, 5, m)]
    off, keys = mk.csr(lists)
    ref = mk.EPaxos(n, NK)
    want = ref.tick(leader, number, [tuple(k) for k in lists], is_set, mask, rank)
    i32 = lambda a: jvm.arr(np.asarray(a, np.int32))
    i8 = lambda a: jvm.arr(np.asarray(a, np.int8))
    fast, deps, ldeps, own = i8(np.zeros(m)), i32(np.zeros(m * n)), i32(np.zeros(m * n)), i32(np.zeros(2 * m))
    st = jvm.call("epxPreacceptMk", C.c_int32, h, m, n, i32(leader), i32(number), i32(off), i32(keys), i8(is_set), i8(mask),
                  None, i32(rank.reshape(-1)), fast, deps, ldeps, own)
    assert st == 0
    F, D, LD, O = (jvm.read(fast, np.int8, m), jvm.read(deps, np.int32, m * n).reshape(m, n),
                   jvm.read(ldeps, np.int32, m * n).reshape(m, n), jvm.read(own, np.int32, 2 * m).reshape(m, 2))
    for i in range(m):
        L, x = int(leader[i]), int(number[i])
        assert bool(F[i]) == want[i][0]
        assert decode(D[i], L, x, O[i][0]) == want[i][1]
        assert decode(LD[i], L, x, O[i][1]) == want[i][2]
    # a Commit of a multi-key set learned from outside, then the index
    st = jvm.call("epxHandleCommitMk", C.c_int32, h, 1, n, i32([3]), i32([NI - 1]), i32([77]), i32([0, 3]), i32([2, 7, 2]),
                  i8([1]), None, None, i8([(1 << n) - 1]))
    assert st == 0
    ref.handle_commit((3, NI - 1), 77, None, range(n), keys=(2, 7, 2), is_set=True)
    from frankenpaxos_amd.epaxos import EPaxos  # noqa: F401  (the binding's read-back of the same handle)
    import frankenpaxos_amd

    L = frankenpaxos_amd.lib()
    for r in range(n):
        for k in range(NK):
            g, s = np.zeros(n, np.int32), np.zeros(n, np.int32)
            assert L.fpx_epx_read_index(C.c_void_p(h), r, k, g.ctypes.data, s.ctypes.data) == 0
            assert g.tolist() == ref.replicas[r].gets[k] and s.tolist() == ref.replicas[r].sets[k]
    assert jvm.call("epxDestroy", C.c_int32, h) == 0
