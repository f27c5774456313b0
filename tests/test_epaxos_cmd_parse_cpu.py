"""The key list of an EPaxos command without a GPU: the host classify (fpx_wire_epx_classify, the parser of
csrc/fpx_epx_cmd_parse.hpp that the device classify runs too) against the parser written a second time in Python
(tests/epaxos_cmd_cases.py), the key table's hash against FNV-1a 64 in Python, and a stand-alone program under the sanitizers:
a mutation fuzz of the parser on heap buffers sized exactly, and the scratch layouts of the new calls."""
import os
import subprocess

import numpy as np
import pytest

from tests import epaxos_cmd_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wire():
    import frankenpaxos_amd
    from frankenpaxos_amd import wire as w

    if not os.path.exists(frankenpaxos_amd._lib.SO_PATH):
        frankenpaxos_amd.build()
    return w


def host_classify(wire, cmds, max_pairs=None, pad=0):
    """the commands back to back (None: no command) through fpx_wire_epx_classify"""
    off, ln, at = [], [], pad
    for c in cmds:
        off.append(-1 if c is None else at), ln.append(-1 if c is None else len(c))
        at += 0 if c is None else len(c)
    buf = np.frombuffer(b"\xff" * pad + b"".join(c for c in cmds if c is not None), np.uint8)
    return wire.epx_classify(buf, off, ln, max_pairs)


def as_expected(out, i=0):
    lo, hi = out["key_offsets"][i], out["key_offsets"][i + 1]
    return (int(out["cmd_shape"][i]), int(out["is_noop"][i]), int(out["is_set"][i]), out["keys"][lo:hi])


@pytest.mark.parametrize("name,msg,want", CC.edge_cases(), ids=[c[0] for c in CC.edge_cases()])
def test_edge_cases(wire, name, msg, want):
    assert CC.parse_command(msg) == want, "the Python parser and the case's expectation"
    out = host_classify(wire, [msg], pad=3)
    if want == CC.MALFORMED:
        assert (out["status_code"], out["bad_index"]) == (1, 0)
    else:
        assert out["status_code"] == 0 and out["bad_index"] == -1
        assert as_expected(out) == want


def test_every_truncation_is_malformed_or_shape_0(wire):
    cuts = CC.truncations()
    assert len(cuts) > 40
    seen = set()
    for j, cut in enumerate(cuts):
        want = CC.parse_command(cut)
        assert want == CC.MALFORMED or want[0] == 0, j
        # the buffer ends with the message: a read past the end leaves the array (the sanitizer run below sees that)
        out = host_classify(wire, [cut])
        if want == CC.MALFORMED:
            assert (out["status_code"], out["bad_index"]) == (1, 0), j
        else:
            assert out["status_code"] == 0 and as_expected(out) == want, j
        seen.add(want if want == CC.MALFORMED else want[0])
    assert seen == {CC.MALFORMED, 0}


@pytest.mark.parametrize("seed,m", [(1, 1), (2, 64), (3, 700), (4, 3000)])
def test_seeded_bursts(wire, seed, m):
    cmds = CC.seeded_burst(seed, m)
    want = CC.classify(cmds)
    out = host_classify(wire, cmds)
    if isinstance(want, tuple):                 # (MALFORMED, the first bad index)
        assert (out["status_code"], out["bad_index"]) == (1, want[1])
        # ... and without the malformed ones the burst classifies
        cmds = [c for c in cmds if c is None or CC.parse_command(c) != CC.MALFORMED]
        want, out = CC.classify(cmds), host_classify(wire, cmds)
    assert out["status_code"] == 0
    for k in ("key_offsets", "is_set", "is_noop", "cmd_shape"):
        assert list(out[k]) == want[k], k
    assert out["keys"] == want["keys"]
    if m >= 700:        # what the burst exercises: every shape, noops, no-command messages, lists of 0, 1 and 5
        assert {-1, 0, 1} <= set(want["cmd_shape"]) and 1 in want["is_noop"] and 1 in want["is_set"]
        lens = set(np.diff(want["key_offsets"]))
        assert {0, 1, 2, 3, 5} <= lens


def test_pair_capacity(wire):
    cmds = [CC.get([b"a", b"b"]), CC.NOOP, CC.set_([b"c"])]
    out = host_classify(wire, cmds, max_pairs=2)
    assert out["status_code"] == 5 and out["key_offsets"][3] == 3
    out = host_classify(wire, cmds, max_pairs=3)
    assert out["status_code"] == 0 and out["keys"] == [b"a", b"b", b"c"]
    # a command outside the buffer is refused like a malformed one
    buf = np.frombuffer(cmds[0], np.uint8)
    for off, ln in ((1, len(cmds[0])), (-2, 3), (len(cmds[0]), 1)):
        out = wire.epx_classify(buf, [0, off], [len(cmds[0]), ln])
        assert (out["status_code"], out["bad_index"]) == (1, 1), (off, ln)


def fnv1a64(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & ((1 << 64) - 1)
    return h


def test_the_hash_is_fnv1a_64(wire):
    # the published test vectors of FNV-1a 64
    assert fnv1a64(b"") == 0xcbf29ce484222325 and fnv1a64(b"a") == 0xaf63dc4c8601ec8c and fnv1a64(b"foobar") == 0x85944171f73967e8
    for key in (b"", b"a", b"foobar", b"k0", b"k1023", bytes(range(256)), b"\x00" * 7, b"x" * 4096):
        assert wire.epx_key_hash(key) == fnv1a64(key), key[:16]


def test_the_parser_fuzz_and_the_scratch_layouts_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "epx_cmd_parse_fuzz")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epx_cmd_parse_fuzz_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    fuzz = [ln for ln in lines if ln.startswith("ok fuzz")]
    assert len(fuzz) == 1
    counts = dict(kv.split("=") for kv in fuzz[0].split()[2:])
    # the mutations reach every verdict, not only "malformed"
    assert int(counts["runs"]) >= 20000 and all(int(counts[k]) > 200 for k in ("canonical", "shape0", "malformed"))
    assert sum(ln.startswith("ok layout") for ln in lines) == 6 * 4 * 3        # m x max_pairs x n


def test_the_binding_and_the_headers_agree():
    import re

    from frankenpaxos_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpx.h")).read(), flags=re.S)
    for name, args in (("fpx_epx_keys_enable", 2), ("fpx_epx_keys_count", 3), ("fpx_epx_keys_intern_dev", 7),
                       ("fpx_epx_keys_intern", 7), ("fpx_epx_keys_read", 6)):
        decl = re.search(r"\b" + name + r"\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(decl.split(",")) == args == len(_lib.SIGNATURES[name][1]), name
    assert "#define FPX_EPX_KEY_MAX_LEN 4096" in code and CC.KEY_MAX_LEN == 4096
    wire_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpx_wire.h")).read(), flags=re.S)
    for name, args in (("fpx_wire_epx_classify", 13), ("fpx_wire_epx_key_hash", 2), ("fpx_wire_epx_classify_dev", 13),
                       ("fpx_wire_epx_replica_tick_dev", 17), ("fpx_wire_epx_replica_tick", 17)):
        decl = re.search(r"\b" + name + r"\(([^)]*)\)", wire_h, flags=re.S).group(1)
        assert len(decl.split(",")) == args, name
