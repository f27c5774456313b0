"""fpx_mencius_proxy_phase2b_msgs / _dev and fpx_mencius_phase2b_tick without a GPU: the symbols are exported, declared
and bound; the argument checks that need no device, through ctypes and through the JNI natives on the mock JVM; and the
streams tests/test_gpu_mencius_phase2b_msgs.py runs are not vacuous -- a condition on the INPUTS, judged by the two
reference models alone (tests/mencius_phase2b_streams.py), which must agree with each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mencius_phase2b_streams as MS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpx_mencius_proxy_phase2b_msgs", "fpx_mencius_proxy_phase2b_msgs_dev", "fpx_mencius_phase2b_tick")
EINVAL = 1


def test_the_three_symbols_are_exported_declared_and_bound():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    L = fa.lib()
    header = open(os.path.join(ROOT, "include", "fpx.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"int32_t " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
    # the prototypes: eleven and fifteen arguments, as declared
    for name, nargs in zip(NAMES, (11, 11, 15)):
        decl = re.search(r"int32_t " + name + r"\(([^)]*)\)", header).group(1)
        assert len(decl.split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    for method in ("mencius_proxy_phase2b_msgs", "mencius_proxy_phase2b_msgs_dev", "mencius_phase2b_tick"):
        assert callable(getattr(fa.Context, method))
    jni = os.path.join(ROOT, "frankenpaxos_amd", "jni")
    scala, shim = open(os.path.join(jni, "Native.scala")).read(), open(os.path.join(jni, "fpx_jni.c")).read()
    for native in ("menciusProxyPhase2bMsgs", "menciusPhase2bTick"):
        assert "def %s(" % native in scala and "Java_frankenpaxos_gpu_Native_%s(" % native in shim
    assert "remoteAcceptors: Boolean = false" in open(os.path.join(jni, "MenciusNative.scala")).read()
    assert "menciusProxyLeaderHandlePhase2bMsgs" in open(os.path.join(ROOT, "frankenpaxos_amd", "host", "fpx.hpp")).read()


def test_null_context_and_negative_n_are_einval_without_a_device():
    import frankenpaxos_amd as fa

    L = fa.lib()
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    for fn in (L.fpx_mencius_proxy_phase2b_msgs, L.fpx_mencius_proxy_phase2b_msgs_dev):
        assert fn(None, 4, None, None, p, p, p, p, None, None, None) == EINVAL
        assert fn(None, -1, None, None, p, p, p, p, None, None, None) == EINVAL
        assert fn(None, 0, None, None, None, None, None, None, None, None, None) == EINVAL
    cnt = C.c_int32(7)
    tick = L.fpx_mencius_phase2b_tick
    assert tick(None, 4, None, None, p, p, p, p, p, p, p, p, p, 4, C.byref(cnt)) == EINVAL
    assert tick(None, -1, None, None, p, p, p, p, p, p, p, p, p, 4, C.byref(cnt)) == EINVAL


def test_the_jni_natives_check_their_arrays_before_native_code_touches_them(jvm):  # noqa: F811
    """every array shorter than the burst needs is FPX_EINVAL; n == 0 is FPX_OK without a context (handle 0)"""
    n = 8
    i32 = lambda k: jvm.arr(np.zeros(k, np.int32))
    i8 = lambda k: jvm.arr(np.zeros(k, np.int8))
    msgs = lambda *a: jvm.call("menciusProxyPhase2bMsgs", C.c_int32, C.c_int64(0), *a)
    ok = (i32(n), i32(n), i32(n), i32(n), i32(n), i32(n))
    assert msgs(n, i32(n), i32(n), i32(n - 1), i32(n), i32(n), i32(n), i8(n), i32(n), i32(n)) == EINVAL   # acceptorIndex
    assert msgs(n, i32(n), i32(n), i32(n), i32(n), i32(n - 1), i32(n), i8(n), i32(n), i32(n)) == EINVAL   # slotEnd
    assert msgs(n, i32(n - 1), i32(n), i32(n), i32(n), i32(n), i32(n), i8(n), i32(n), i32(n)) == EINVAL   # kind
    assert msgs(n, *ok, i8(n - 1), i32(n), i32(n)) == EINVAL
    assert msgs(n, *ok, i8(n), i32(n), i32(n - 1)) == EINVAL
    assert msgs(n, None, None, None, i32(n), None, i32(n), None, None, None) == EINVAL                    # no acceptorIndex
    assert msgs(-1, *ok, None, None, None) == EINVAL
    assert msgs(0, None, None, None, None, None, None, None, None, None) == 0
    tick = lambda *a: jvm.call("menciusPhase2bTick", C.c_int32, C.c_int64(0), *a)
    outs = lambda k: (i32(k), i32(k), i32(k), i32(k), i32(k))
    assert tick(n, *ok, *outs(4), 4, None) == EINVAL                                                      # no outCount
    assert tick(n, *ok, *outs(4), 4, i32(0)) == EINVAL
    assert tick(n, *ok, *outs(3), 4, i32(1)) == EINVAL
    assert tick(n, *ok, i32(4), i32(4), None, i32(4), i32(4), 4, i32(1)) == EINVAL
    assert tick(n, i32(n), i32(n), i32(n), i32(n - 1), i32(n), i32(n), *outs(4), 4, i32(1)) == EINVAL     # slot
    assert tick(n, *ok, *outs(4), -1, i32(1)) == EINVAL
    assert tick(-1, *ok, *outs(4), 4, i32(1)) == EINVAL


@pytest.fixture(scope="module")
def models():
    from oracle import mencius_maps, pyoracle

    pyoracle.build()
    return pyoracle, mencius_maps


@pytest.mark.parametrize("shape", sorted(MS.SHAPES))
@pytest.mark.parametrize("layout", MS.LAYOUTS)
def test_the_models_agree_and_the_streams_are_not_vacuous(models, shape, layout):
    pyoracle, mencius_maps = models
    st = MS.Stream(shape, 20000, layout, seed=7)
    assert st.n == 20000 and len(st.kind) == 20000
    kw, A = st.kw, st.kw["num_groups"]
    # the rows path on the oracle, one burst
    ref = pyoracle.System(pyoracle.make_config(**kw))
    MS.open_all(ref, st)
    d = st.decoded()
    rc, ch, cr, cv = MS.rows_path(ref, d, kw)
    assert rc == 0
    rows_chosen = MS.chosen_keys(d, ch)
    # the message-at-a-time path
    chosen, decided, states = MS.maps_run(mencius_maps, st)
    assert sorted(rows_chosen) == sorted(chosen) and len(set(chosen)) == len(chosen)
    range_keys = [k for k in st.range_keys() if k not in st.swallowed]
    for k in range_keys:
        assert ref.read_range_tally(*k)[0] == states[k], k
    for s in sorted(set(st.single_slot.tolist())):
        for rnd, state, value, bits in ref.read_tally(s):
            if (s, rnd) not in st.shadowed:
                assert states[(s, s + 1, rnd)] - 1 == state, (s, rnd)   # read_tally: 0 Pending, 1 Done
    # not vacuous
    done = [k for k in range_keys if states[k] == 2]
    assert 5 * len(done) >= len(range_keys), (len(done), len(range_keys))
    assert 5 * (len(range_keys) - len(done)) >= len(range_keys), (len(range_keys) - len(done), len(range_keys))
    is_range = st.kind == MS.RANGE
    assert is_range.any() and (st.kind == MS.PHASE2B).any()
    assert len(done) > 0 and len(chosen) > len(done)                # both kinds get chosen
    if A > 1:   # a quorum in some acceptor group but not in all
        _, rrows = MS.fold(d, kw)
        partial = 0
        for _, s, e, r, bits in rrows:
            full = [sum(bin(int(w)).count("1") for w in bits[g]) >= kw["f"] + 1 for g in range(A)]
            partial += any(full) and not all(full)
        assert partial > 0
    # duplicates: a message whose (kind, key, group, acceptor) came before
    seen, dups = set(), 0
    for m in zip(st.kind.tolist(), st.slot.tolist(), st.slot_end.tolist(), st.round.tolist(), st.group_index.tolist(),
                 st.acceptor_index.tolist()):
        dups += m in seen
        seen.add(m)
    assert 20 * dups >= st.n, dups
    # a Done range gets a vote after the message that completed it
    late = sum(1 for i, (k, s, e, r) in enumerate(zip(st.kind.tolist(), st.slot.tolist(), st.slot_end.tolist(), st.round.tolist()))
               if k == MS.RANGE and decided.get((s, e, r), st.n) < i)
    assert late > 0
    # the directed ranges are there: no row, one slot, ends at S, two rounds of one range, a key a single slot holds
    lens = (st.range_end - st.range_start).tolist()
    assert 0 in lens and 1 in lens and kw["num_slots"] in st.range_end.tolist() and st.swallowed and st.shadowed
    pairs = {}
    for s, e, r in st.range_keys():
        pairs.setdefault((s, e), set()).add(r)
    assert any(len(v) > 1 for v in pairs.values())
