"""A replica's inbox from wire bytes: what the host does today in front of fpx_epx_replica_inbox_mk -- decode, classify, a
hash map for the key ids -- against the tick that does all of it on the device.  The numbers of
profiles/epx_wire_replica_tick.md.

    python profiles/microbench/epx_wire_replica_tick.py [--keys-each 1 | 4] [--messages N]

The burst: n = 5, `messages` serialised PreAccepts (default 2^20), instance j = (j % 5, j / 5) in its leader's default ballot,
received by the leader's right neighbour; every command a get (even j) or a set (odd j) over keys drawn from 1 024 distinct
decimal strings ("0" .. "1023"), one key each or 1 - 4 keys each; empty dependencies.  Bytes, offsets and `to` in page-locked
memory (fpx_host_alloc).
  (a) the yardstick, what the parent commit offers for the same frames: fpx_wire_epaxos_decode_replica_inbound_folded (one
      host thread) + the kind map, a host classify built from the same parser header with a std::unordered_map<std::string,
      int> (profiles/microbench/epx_classify_host.cpp), fpx_epx_replica_inbox_mk; the three shares separately
  (b) fpx_wire_epx_replica_tick: copy up, decode + check + classify + intern on the device, one host wait, the inbox's
      kernels, copy down
  (c) fpx_wire_epx_replica_tick_dev, the bytes already in HBM
  and its parts on their own, device-resident: (d) fpx_wire_epaxos_decode_replica_inbound_dev, (e)
  fpx_wire_epx_classify_dev on the decoded cmd_off / cmd_len (first call: the keys are new; again: all resident), (f)
  fpx_epx_replica_inbox_mk_dev on the decoded arrays
  (g) the intern step alone, fpx_epx_keys_intern_dev on 2^20 strings: over 1 024 distinct keys and over 2^19 distinct keys in
      a table of num_keys = 2^19 (half its slots end up full); first batch (the keys are new) and again (all resident)
(a) and (b) are synchronous calls timed by the host clock on fresh contexts; (c) - (g) between two HIP events on the
context's stream, enqueue to fpx_epx_sync.  The median of --bursts after --warmup.  The outputs of (b) and (c) are compared
with (a)'s after the timed region.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
N = 5
DISTINCT = 1024


def varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def ld(field, body):
    return varint(field << 3 | 2) + varint(len(body)) + body


def i32(field, v):
    return varint(field << 3) + varint(v)


def build_burst(m, keys_each, seed=4):
    """(bytes, offsets, to, the first 64 commands): the PreAccepts back to back, assembled from a pool of 4 096 commands"""
    rng = np.random.default_rng(seed)
    pool, cmds = [], []
    for c in range(4096):
        k = 1 if keys_each == 1 else 1 + int(rng.integers(0, keys_each))
        ks = [b"%d" % int(rng.integers(0, DISTINCT)) for _ in range(k)]
        req = ld(2, b"".join(ld(1, ld(1, x) + ld(2, b"v")) for x in ks)) if c & 1 else ld(1, b"".join(ld(1, x) for x in ks))
        cmd = ld(1, ld(1, b"\x0a\x00\x00\x01") + i32(2, 1) + i32(3, c) + ld(4, req))
        pool.append(ld(3, cmd))
        cmds.append(cmd)
    deps = ld(5, i32(1, N) + ld(2, i32(1, 0)) * N)
    tail = [ld(2, i32(1, 0) + i32(2, L)) for L in range(N)]
    pick = rng.integers(0, 2048, m) * 2 + (np.arange(m) & 1)      # even j a get, odd j a set
    frames = []
    for j in range(m):
        L = j % N
        body = ld(1, i32(1, L) + i32(2, j // N)) + tail[L] + pool[pick[j]] + b"\x20\x00" + deps
        frames.append(b"\x12" + varint(len(body)) + body)
    off = np.zeros(m + 1, np.int64)
    np.cumsum([len(f) for f in frames], out=off[1:])
    to = ((np.arange(m) % N + 1) % N).astype(np.int32)
    return np.frombuffer(b"".join(frames), np.uint8).copy(), off, to, [cmds[p] for p in pick[:64]]


class Cfg(C.Structure):
    _fields_ = [("num_replicas", C.c_int32), ("num_keys", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("num_instances", C.c_int32)]


def host_classify_lib():
    out = os.path.join(HERE, "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libepx_classify_host.so")
    src = os.path.join(HERE, "epx_classify_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.mb_classify.restype = C.c_int64
    L.mb_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--keys-each", type=int, default=1, choices=[1, 4])
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-intern", action="store_true")
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd import wire

    lib = wire._L()
    host = host_classify_lib()
    m = a.messages
    per = (m + N - 1) // N
    buf, off, to, first_cmds = build_burst(m, a.keys_each)
    in_len = int(off[-1])
    # the hand-assembled frames are what the library's encoder writes
    for j, cmd in enumerate(first_cmds):
        want = wire.epaxos_encode(wire.EPX_PRE_ACCEPT, (j % N, j // N), (0, j % N), sequence_number=0, deps=[0] * N, command=cmd)
        assert want == buf[off[j]:off[j + 1]].tobytes(), j
    max_pairs = a.keys_each * m

    def locked(arr):
        p = C.c_void_p()
        assert lib.fpx_host_alloc(max(arr.nbytes, 8), C.byref(p)) == 0
        C.memmove(p, arr.ctypes.data, arr.nbytes)
        return p

    h_buf, h_off, h_to = locked(buf), locked(off), locked(to)
    stream = torch.cuda.Stream()
    hp = lambda v: C.c_void_p(v.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def fresh(num_keys=DISTINCT, instances=per, arena=1 << 16, n=N):
        h = C.c_void_p()
        cfg = Cfg(n, num_keys, 0, 0, instances)
        assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
        assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        assert lib.fpx_epx_keys_enable(h, arena) == 0
        return h

    i32a = lambda k: np.zeros(k, np.int32)
    outs = lambda: dict(outcome=i32a(m), ob=i32a(m), os=i32a(m), odeps=i32a(m * N), oend=i32a(m), otr=i32a(m))
    out_args = lambda o: [hp(o[k]) for k in ("outcome", "ob", "os", "odeps", "oend", "otr")]
    names = wire.EPX_FOLDED_NAMES
    dec = {k: (np.zeros(m, np.int64) if k == "cmd_off" else i32a(m * N if k == "deps_watermark" else m)) for k in names}
    lut = np.full(32, -1, np.int32)
    lut[[wire.EPX_PRE_ACCEPT, wire.EPX_ACCEPT, wire.EPX_COMMIT, wire.EPX_PREPARE]] = [0, 1, 2, 3]
    koff, keys, iset = i32a(m + 1), i32a(max_pairs), np.zeros(m, np.uint8)
    tid = np.arange(m, dtype=np.int32)
    t = {k: [] for k in ("a_decode", "a_classify", "a_inbox", "a", "b", "c", "d_decode", "e_classify_new", "e_classify_resident",
                         "f_inbox")}
    with torch.cuda.stream(stream):
        d_buf, d_off, d_to = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(to).cuda()
        d_out = [torch.zeros(m * (N if k == 3 else 1), dtype=torch.int32, device="cuda") for k in range(6)]
        d_res = torch.zeros(4, dtype=torch.int32, device="cuda")
        d_dec = {k: torch.zeros(m * N if k == "deps_watermark" else m, dtype=torch.int64 if k == "cmd_off" else torch.int32,
                                device="cuda") for k in names}
        d_koff = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        d_keys = torch.zeros(max_pairs, dtype=torch.int32, device="cuda")
        d_iset = torch.zeros(m, dtype=torch.uint8, device="cuda")
        d_noop, d_shape, d_kind = (torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3))
        d_tid = torch.from_numpy(tid).cuda()
    stream.synchronize()

    def timed_dev(fn, h):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert fn() == 0
        assert lib.fpx_epx_sync(h) == 0
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {}
    for it in range(a.warmup + a.bursts):
        keep = it >= a.warmup
        # (a) decode on the host, classify on the host, the inbox call
        h = fresh()
        oa = outs()
        bad = C.c_int32(-1)
        host.mb_reset()
        t0 = time.perf_counter()
        st = lib.fpx_wire_epaxos_decode_replica_inbound_folded(h_buf, in_len, h_off, m, N, *[hp(dec[k]) for k in names], C.byref(bad))
        assert st == 0
        kind = lut[dec["kind"]]
        t1 = time.perf_counter()
        P = host.mb_classify(h_buf, hp(dec["cmd_off"]), hp(dec["cmd_len"]), m, hp(koff), hp(keys), hp(iset), max_pairs)
        t2 = time.perf_counter()
        assert 0 < P <= max_pairs
        st = lib.fpx_epx_replica_inbox_mk(h, m, hp(kind), h_to, hp(dec["instance_leader"]), hp(dec["instance_number"]),
                                          hp(dec["ballot_ordering"]), hp(dec["ballot_replica"]), hp(koff), hp(keys), hp(iset), hp(tid),
                                          hp(dec["deps_watermark"]), hp(dec["deps_values_end"]), *out_args(oa))
        t3 = time.perf_counter()
        assert st == 0
        assert lib.fpx_epx_destroy(h) == 0
        # (b) the tick, host pointers
        h = fresh()
        ob = outs()
        bad, npairs = C.c_int32(-9), C.c_int32(-9)
        t4 = time.perf_counter()
        st = lib.fpx_wire_epx_replica_tick(h, h_buf, in_len, h_off, m, h_to, 0, None, max_pairs, *out_args(ob), C.byref(bad),
                                           C.byref(npairs))
        t5 = time.perf_counter()
        assert st == 0 and bad.value == -1 and npairs.value == P, (st, bad.value, npairs.value, P)
        assert lib.fpx_epx_destroy(h) == 0
        for k in oa:
            assert (oa[k] == ob[k]).all(), k
        # (c) the tick, the bytes in HBM
        h = fresh()
        ms_c = timed_dev(lambda: lib.fpx_wire_epx_replica_tick_dev(h, dp(d_buf), in_len, dp(d_off), m, dp(d_to), 0, None, max_pairs,
                                                                   *[dp(x) for x in d_out], dp(d_res[0:1]), dp(d_res[1:2])), h)
        assert d_res[:2].tolist() == [-1, P]
        for k, x in zip(("outcome", "ob", "os", "odeps", "oend", "otr"), d_out):
            assert (x.cpu().numpy() == oa[k]).all(), k
        assert lib.fpx_epx_destroy(h) == 0
        # (d), (e), (f): the parts, device-resident
        h = fresh()
        ms_d = timed_dev(lambda: lib.fpx_wire_epaxos_decode_replica_inbound_dev(h, dp(d_buf), in_len, dp(d_off), m,
                                                                                *[dp(d_dec[k]) for k in names], dp(d_res[0:1])), h)
        cls = lambda: lib.fpx_wire_epx_classify_dev(h, dp(d_buf), in_len, dp(d_dec["cmd_off"]), dp(d_dec["cmd_len"]), m, max_pairs,
                                                    dp(d_koff), dp(d_keys), dp(d_iset), dp(d_noop), dp(d_shape), dp(d_res))
        ms_e1 = timed_dev(cls, h)
        assert d_res.tolist()[:3] == [-1, P, host.mb_count()]
        ms_e2 = timed_dev(cls, h)
        assert d_res.tolist()[1:] == [P, 0, 0] and (d_keys[:P].cpu().numpy() == keys[:P]).all()
        d_kind.copy_(torch.from_numpy(kind))
        ms_f = timed_dev(lambda: lib.fpx_epx_replica_inbox_mk_dev(
            h, m, dp(d_kind), dp(d_to), dp(d_dec["instance_leader"]), dp(d_dec["instance_number"]), dp(d_dec["ballot_ordering"]),
            dp(d_dec["ballot_replica"]), dp(d_koff), dp(d_keys), P, dp(d_iset), dp(d_tid), dp(d_dec["deps_watermark"]),
            dp(d_dec["deps_values_end"]), *[dp(x) for x in d_out]), h)
        assert (d_out[0].cpu().numpy() == oa["outcome"]).all()
        assert lib.fpx_epx_destroy(h) == 0
        if keep:
            t["a_decode"].append((t1 - t0) * 1e3), t["a_classify"].append((t2 - t1) * 1e3), t["a_inbox"].append((t3 - t2) * 1e3)
            t["a"].append((t3 - t0) * 1e3), t["b"].append((t5 - t4) * 1e3), t["c"].append(ms_c), t["d_decode"].append(ms_d)
            t["e_classify_new"].append(ms_e1), t["e_classify_resident"].append(ms_e2), t["f_inbox"].append(ms_f)
        res = dict(pairs=int(P), distinct_keys=host.mb_count(), pre_accept_ok=int((oa["outcome"] == 1).sum()))
    out = dict(n=N, messages=m, keys_each=a.keys_each, bytes=in_len, bytes_per_message=round(in_len / m, 2), bursts=a.bursts, **res)
    for k, v in t.items():
        med = statistics.median(v)
        out[k] = dict(ms_median=round(med, 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), msgs_per_s=round(m / med * 1e3))
    # (g) the intern step alone
    if not a.skip_intern:
        S = 1 << 20
        rng = np.random.default_rng(9)
        for name, distinct, num_keys in (("g_intern_1024", DISTINCT, DISTINCT), ("g_intern_2p19", 1 << 19, 1 << 19)):
            ids = np.concatenate([rng.permutation(distinct), rng.integers(0, distinct, S - distinct)]) if distinct < S else None
            rng.shuffle(ids)
            strs = np.char.encode(ids.astype("U"), "ascii")
            ln = np.char.str_len(strs).astype(np.int32)
            koff64 = np.zeros(S, np.int64)
            np.cumsum(ln[:-1], out=koff64[1:])
            kb = np.frombuffer(b"".join(strs.tolist()), np.uint8).copy()
            with torch.cuda.stream(stream):
                d_kb, d_ko, d_kl = torch.from_numpy(kb).cuda(), torch.from_numpy(koff64).cuda(), torch.from_numpy(ln).cuda()
                d_ids = torch.zeros(S, dtype=torch.int32, device="cuda")
            stream.synchronize()
            new, again = [], []
            for it in range(a.warmup + a.bursts):
                h = fresh(num_keys=num_keys, instances=0, arena=1 << 23, n=3)
                call = lambda: lib.fpx_epx_keys_intern_dev(h, dp(d_kb), len(kb), dp(d_ko), dp(d_kl), S, dp(d_ids))
                ms1, ms2 = timed_dev(call, h), timed_dev(call, h)
                got = d_ids.cpu().numpy()
                _, first = np.unique(ids, return_index=True)
                assert got.max() == distinct - 1 and (got[np.sort(first)] == np.arange(distinct)).all()   # first-occurrence order
                assert lib.fpx_epx_destroy(h) == 0
                if it >= a.warmup:
                    new.append(ms1), again.append(ms2)
            for tag, v in (("new", new), ("resident", again)):
                med = statistics.median(v)
                out["%s_%s" % (name, tag)] = dict(ms_median=round(med, 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                                                  strings=S, distinct=distinct, keys_per_s=round(S / med * 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
