"""The command store on the steady burst, and its put alone.  The numbers of profiles/epx_wire_replica_cmds.md.

    python profiles/microbench/epx_wire_replica_cmds.py [--messages N] [--bursts B]

The burst is profiles/microbench/epx_wire_replica_tick.py's: n = 5, `messages` serialised PreAccepts (default 2^20), one key
each, every one answered with a PreAcceptOk.  Bytes, offsets and `to` in page-locked memory.
  (a) fpx_wire_epx_replica_tick_bytes, host form, no struct-of-arrays output, on a fresh context: without the store, with the
      store in its `bytes` copy form (the default) and in its `words` form (FPX_EPX_CMDS_WORDS), alternated; synchronous calls timed by
      the host clock.  With the store every PreAccept's command goes into the arena behind stage 2.
  (b) recovery: the same instances stored as Accepted (the burst again as Accepts, untimed), then `messages` Prepares in a
      higher ballot, every one answered with a PrepareOk(Accepted) that carries the stored command.  With the store: the bytes
      tick alone, no struct-of-arrays output.  Without it, the parent commit's path: the bytes tick with all six arrays (every
      reply comes back deferred), then ONE host thread encoding them -- here with a single call of the host batch encoder
      fpx_wire_epx_encode_replica_replies_cmds over the whole burst, which is cheaper than the parent's one call per message
      (no per-call setup, no message struct): the bar is set high.  The two paths' bytes are compared.
  (c) fpx_epx_cmds_put_dev alone, device-resident, on the commands of the same burst (located by the host decoder), and
      fpx_wire_epx_encode_replica_replies_cmds_dev alone on the Prepares' records in HBM, both copy forms: enqueue to
      fpx_epx_sync between two HIP events, the fastest of three calls (the put: each on a fresh store whose scratch is sized),
      as bytes moved per second.
Median, minimum and maximum of --bursts after --warmup.  One JSON line.
  --tree DIR   import frankenpaxos_amd from DIR, a built checkout of ANOTHER commit (the parent's), in place of this one: only
               the tick of (a) without the store is timed then -- the rest needs this commit's entry points.  Run for both
               trees in turn within one session, it is the comparison of the no-store tick with the parent's."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
N = 5
REPLY_MAX = 472
FORMS = ("none", "words", "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tree", default=None, help="a built checkout of another commit: time its no-store tick of (a) alone")
    a = ap.parse_args()
    only_a = a.tree is not None
    forms = ("none",) if only_a else FORMS
    import epx_wire_replica_tick as SIB  # the sibling profile's burst

    m = a.messages
    buf, off, to, _ = SIB.build_burst(m, 1)
    in_len = int(off[-1])
    import torch  # the HIP runtime both sides share: before anything that loads libfpx.so

    if only_a:
        sys.path.insert(0, os.path.abspath(a.tree))           # (in front of this checkout's root, which the sibling put there)
    from frankenpaxos_amd import wire

    lib = wire._L()
    assert not only_a or os.path.abspath(wire._lib.SO_PATH).startswith(os.path.abspath(a.tree) + os.sep), wire._lib.SO_PATH
    per = (m + N - 1) // N
    cap = m * REPLY_MAX
    # the commands of the burst, as the tick's decoder locates them
    step = 1 << 16
    cmd_off, cmd_len = np.zeros(m, np.int64), np.zeros(m, np.int32)
    for lo in range(0, 0 if only_a else m, step):
        hi = min(m, lo + step)
        frames = [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(lo, hi)]
        dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=N)
        assert dec["status_code"] == 0
        cmd_off[lo:hi], cmd_len[lo:hi] = dec["cmd_off"] + int(off[lo]), dec["cmd_len"]
    cmd_bytes = int(cmd_len.sum())
    # (b): the burst as Accepts (the same layout under ReplicaInbound's field 4), and a Prepare per instance in ballot (1, leader)
    acc = buf.copy()
    assert (acc[off[:-1]] == 0x12).all()
    acc[off[:-1]] = 0x22
    prep = [SIB.ld(7, SIB.ld(1, SIB.i32(1, j % N) + SIB.i32(2, j // N)) + SIB.ld(2, SIB.i32(1, 1) + SIB.i32(2, j % N)))
            for j in range(1 if only_a else m)]
    poff = np.zeros(len(prep) + 1, np.int64)
    np.cumsum([len(f) for f in prep], out=poff[1:])
    pbuf = np.frombuffer(b"".join(bytes(f) for f in prep), np.uint8).copy()
    p_len = int(poff[-1])
    leader = (np.arange(m) % N).astype(np.int32)
    number = (np.arange(m) // N).astype(np.int32)
    b_ord, b_rep = np.ones(m, np.int32), leader.copy()
    arena = cmd_bytes + 64

    def locked(arr):
        p = C.c_void_p()
        assert lib.fpx_host_alloc(max(arr.nbytes, 8), C.byref(p)) == 0
        C.memmove(p, arr.ctypes.data, arr.nbytes)
        return p

    h_buf, h_off, h_to = locked(buf), locked(off), locked(to)
    h_acc, h_pbuf, h_poff = locked(acc), locked(pbuf), locked(poff)
    stream = torch.cuda.Stream()
    hp = lambda v: C.c_void_p(v.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def fresh(form):
        os.environ.pop("FPX_EPX_CMDS_WORDS", None)
        if form == "words":
            os.environ["FPX_EPX_CMDS_WORDS"] = "1"
        h = C.c_void_p()
        cfg = SIB.Cfg(N, SIB.DISTINCT, 0, 0, per)
        assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
        os.environ.pop("FPX_EPX_CMDS_WORDS", None)
        assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        assert lib.fpx_epx_keys_enable(h, 1 << 16) == 0
        if form != "none":
            assert lib.fpx_epx_cmds_enable(h, m, arena) == 0
        return h

    out2, off2, kind2, tot2 = np.zeros(cap, np.uint8), np.zeros(m + 1, np.int64), np.zeros(m, np.uint8), np.zeros(4, np.int64)
    stats = np.zeros(4, np.int64)
    t = {"a_bytes_tick_%s" % f: [] for f in FORMS}
    t.update({"c_put_%s" % f: [] for f in FORMS[1:]})
    t.update({"c_encoder_%s" % f: [] for f in FORMS[1:]})
    t.update({k: [] for k in ("b_parent_tick", "b_parent_host_encode", "b_parent_path", "b_store_tick_words", "b_store_tick_bytes")})
    i32a = lambda k: np.zeros(k, np.int32)
    soa = [i32a(m), i32a(m), i32a(m), i32a(m * N), i32a(m), i32a(m)]   # outcome, out_ballot, out_status, out_deps, out_values_end, out_triple
    out1, off1, kind1, tot1 = np.zeros(cap, np.uint8), np.zeros(m + 1, np.int64), np.zeros(m, np.uint8), np.zeros(4, np.int64)
    reply_bytes = 0
    with torch.cuda.stream(stream):
        d_buf, d_off, d_len = (torch.from_numpy(x).cuda() for x in (buf, cmd_off, cmd_len))
        d_tr = torch.arange(m, dtype=torch.int32, device="cuda")
        d_skip = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(4, dtype=torch.int64, device="cuda")
    stream.synchronize()

    def timed_dev(fn, h):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert fn() == 0
        assert lib.fpx_epx_sync(h) == 0
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ref = None
    for it in range(a.warmup + a.bursts):
        keep = it >= a.warmup
        order = forms if it % 2 == 0 else forms[::-1]
        for form in order:
            h = fresh(form)
            bad, npairs = C.c_int32(-9), C.c_int32(-9)
            t0 = time.perf_counter()
            st = lib.fpx_wire_epx_replica_tick_bytes(h, h_buf, in_len, h_off, m, h_to, 0, None, m, hp(out2), cap, hp(off2), hp(kind2),
                                                     hp(tot2), *([None] * 6), C.byref(bad), C.byref(npairs))
            t1 = time.perf_counter()
            assert st == 0 and tot2[0] == m and tot2[2] == 0, (st, tot2.tolist())
            if ref is None:
                ref = (off2.copy(), out2[:int(tot2[1])].copy())
            assert (off2 == ref[0]).all() and out2[:int(tot2[1])].tobytes() == ref[1].tobytes()
            if form != "none":
                assert lib.fpx_epx_cmds_stats(h, hp(stats)) == 0 and stats.tolist() == [m, cmd_bytes, 0, 0], stats.tolist()
            assert lib.fpx_epx_destroy(h) == 0
            if keep:
                t["a_bytes_tick_%s" % form].append((t1 - t0) * 1e3)
        for form in order:
            if form == "none":
                continue
            ms = []
            for _ in range(3):
                h = fresh(form)
                put = lambda ids: lib.fpx_epx_cmds_put_dev(h, dp(d_buf), in_len, dp(d_off), dp(d_len), dp(ids), m, dp(d_res))
                # (a put of m records that are not considered sizes the scratch and loads the code objects: the store stays fresh)
                timed_dev(lambda: put(d_skip), h)
                ms.append(timed_dev(lambda: put(d_tr), h))
                assert d_res.tolist() == [m, cmd_bytes, 0, 0], d_res.tolist()
                assert lib.fpx_epx_destroy(h) == 0
            if keep:
                t["c_put_%s" % form].append(min(ms))
        # (b) and the encoder of (c): every instance stored as Accepted, then the Prepares
        for form in (() if only_a else order):
            h = fresh(form)
            bad, npairs = C.c_int32(-9), C.c_int32(-9)
            st = lib.fpx_wire_epx_replica_tick_bytes(h, h_acc, in_len, h_off, m, h_to, 0, None, m, hp(out2), cap, hp(off2), hp(kind2),
                                                     hp(tot2), *([None] * 6), C.byref(bad), C.byref(npairs))
            assert st == 0 and tot2[0] == m, (st, tot2.tolist())            # an AcceptOk each
            want_soa = form == "none"
            t0 = time.perf_counter()
            st = lib.fpx_wire_epx_replica_tick_bytes(h, h_pbuf, p_len, h_poff, m, h_to, 0, None, m, hp(out2), cap, hp(off2), hp(kind2),
                                                     hp(tot2), *([hp(x) for x in soa] if want_soa else [None] * 6), C.byref(bad),
                                                     C.byref(npairs))
            t1 = time.perf_counter()
            assert st == 0, (st, bad.value)
            if form == "none":
                assert tot2.tolist()[0] == 0 and tot2[2] == m and (soa[0] == 6).all() and (soa[2] == 3).all()
                # the parent's path goes on: one host thread, the commands where the frames left them (triple i = message i)
                st = lib.fpx_wire_epx_encode_replica_replies_cmds(
                    N, m, *[hp(x) for x in (to, leader, number, b_ord, b_rep, soa[0], soa[1], soa[2], soa[3], soa[4], soa[5])],
                    hp(cmd_off), hp(cmd_len), hp(buf), m, hp(out1), cap, hp(off1), hp(kind1), hp(tot1))
                t2 = time.perf_counter()
                assert st == 0 and tot1[0] == m and tot1[2] == 0, (st, tot1.tolist())
                reply_bytes = int(tot1[1])
                if keep:
                    t["b_parent_tick"].append((t1 - t0) * 1e3), t["b_parent_host_encode"].append((t2 - t1) * 1e3)
                    t["b_parent_path"].append((t2 - t0) * 1e3)
            else:
                assert tot2.tolist() == [m, reply_bytes, 0, -1] or reply_bytes == 0, tot2.tolist()
                if reply_bytes:
                    assert (off2 == off1).all() and out2[:reply_bytes].tobytes() == out1[:reply_bytes].tobytes()
                if keep:
                    t["b_store_tick_%s" % form].append((t1 - t0) * 1e3)
                if reply_bytes:
                    # the encoder alone on the Prepares' records in HBM, this context's store behind it
                    with torch.cuda.stream(stream):
                        d_rec = [torch.from_numpy(x).cuda() for x in (to, leader, number, b_ord, b_rep, *soa)]
                        d_out = torch.zeros(reply_bytes, dtype=torch.uint8, device="cuda")
                        d_oo = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
                        d_kind = torch.zeros(m, dtype=torch.uint8, device="cuda")
                        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
                    stream.synchronize()
                    enc = lambda: lib.fpx_wire_epx_encode_replica_replies_cmds_dev(h, m, *[dp(x) for x in d_rec], dp(d_out), reply_bytes,
                                                                                   dp(d_oo), dp(d_kind), dp(d_tot))
                    ms = [timed_dev(enc, h) for _ in range(4)][1:]
                    assert d_tot.tolist() == [m, reply_bytes, 0, -1] and d_out.cpu().numpy().tobytes() == out1[:reply_bytes].tobytes()
                    if keep:
                        t["c_encoder_%s" % form].append(min(ms))
                    del d_rec, d_out, d_oo, d_kind, d_tot
            assert lib.fpx_epx_destroy(h) == 0
    out = dict(n=N, messages=m, in_bytes=in_len, command_bytes=cmd_bytes, command_bytes_per_message=round(cmd_bytes / m, 2),
               bursts=a.bursts, library=wire._lib.SO_PATH if hasattr(wire, "_lib") else "")
    for k, v in t.items():
        if not v:
            continue
        med = statistics.median(v)
        out[k] = dict(ms_median=round(med, 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), msgs_per_s=round(m / med * 1e3))
    if only_a:
        print(json.dumps(out))
        return
    out["reply_bytes"] = reply_bytes
    # what the put must move, term by term.  Per record: cmd_len 4 B and triple_id 4 B in each of the four passes that look at a
    # record (claim, length, copy, release) and cmd_off 8 B in the copy pass = 40 B read; the scan word 4 B written by the
    # length pass, 4 B read and 4 B written by the scan, 4 B read by the copy pass = 16 B; the claim word 4 B written, read
    # twice and written back = 16 B; off 8 B + len 4 B written for a writer = 12 B.  And the command bytes, read and written
    moved = 2 * cmd_bytes + (40 + 16 + 16 + 12) * m
    for form in FORMS[1:]:
        ms = out["c_put_%s" % form]["ms_median"]
        out["c_put_%s" % form].update(bytes_moved=moved, gb_per_s=round(moved / ms / 1e6, 1),
                                     command_gb_per_s=round(2 * cmd_bytes / ms / 1e6, 1))
    # the encoder: the eleven record arrays ((10 + n) x 4 B per record) read by the length pass and again by the emit pass, off
    # 8 B and len 4 B of the store per pass, the scan word as above (16 B), offsets 8 B and kind 1 B written; the reply bytes
    # written and the command bytes read
    enc_moved = reply_bytes + cmd_bytes + (2 * (10 + N) * 4 + 2 * 12 + 16 + 9) * m
    for form in FORMS[1:]:
        ms = out["c_encoder_%s" % form]["ms_median"]
        out["c_encoder_%s" % form].update(bytes_moved=enc_moved, gb_per_s=round(enc_moved / ms / 1e6, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
