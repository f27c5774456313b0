"""A replica tick's replies as wire bytes: what a caller of fpx_wire_epx_replica_tick does today with the tick's struct-of-arrays
outputs -- one fpx_wire_epaxos_encode_replica_inbound call per message on one host thread -- against the tick that encodes
them on the device.  The numbers of profiles/epx_wire_replica_replies.md.

    python profiles/microbench/epx_wire_replica_replies.py [--messages N] [--bursts B]

The burst is profiles/microbench/epx_wire_replica_tick.py's: n = 5, `messages` serialised PreAccepts (default 2^20), one key
each, every one answered with a PreAcceptOk.  Bytes, offsets and `to` in page-locked memory.
  (1) the parent's path: fpx_wire_epx_replica_tick (host form), then the per-message encode loop of
      profiles/microbench/epx_reply_host.cpp over its outputs.  The loop is handed the decoded instance and ballot of every
      message for nothing (a caller that holds raw frames would have to parse them out first): the bar is set low
  (2) fpx_wire_epx_replica_tick_bytes, host form, no struct-of-arrays output requested; and (2s) with all six requested
  (3) the encoder alone, device-resident (fpx_wire_epx_encode_replica_replies_dev on the tick's outputs in HBM), in both emit
      forms of csrc/fpx_wire_epx_enc_dev.hpp: `span` (LDS slots, aligned 16-byte stores) and `direct` (FPX_EPX_ENC_DIRECT:
      every lane writes its reply byte by byte), alternated within one run
  (4) the bytes each path copies down, counted from the sizes
(1) and (2) are synchronous calls timed by the host clock, alternated, each on a fresh context (`first`: the PreAccepts are new;
the call also grows the context's buffers) and then the same burst again on that context (`again`: the buffers are sized, every
message is answered with the stored PreAcceptOk again); (3) between two HIP events on the context's stream, enqueue to
fpx_epx_sync, the fastest of three calls.  Median, minimum and maximum of --bursts after --warmup.  The bytes of (2) and (3)
are compared with (1)'s after the timed region.  One JSON line."""
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
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
N = 5
REPLY_MAX = 472


def host_encode_lib():
    out = os.path.join(HERE, "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libepx_reply_host.so")
    src = os.path.join(HERE, "epx_reply_host.cpp")
    csrc = os.path.join(ROOT, "frankenpaxos_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src, "-L" + csrc, "-lfpx",
                               "-Wl,-rpath," + csrc])
    L = C.CDLL(so)
    L.mb_encode_replies.restype = C.c_int64
    L.mb_encode_replies.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 11 + [C.c_int64, C.c_void_p, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--build-only", action="store_true", help="build the host yardstick and the burst, touch no device")
    a = ap.parse_args()
    import epx_wire_replica_tick as SIB  # the sibling profile's burst

    m = a.messages
    buf, off, to, _ = SIB.build_burst(m, 1)
    in_len = int(off[-1])
    leader = (np.arange(m) % N).astype(np.int32)
    number = (np.arange(m) // N).astype(np.int32)
    b_ord, b_rep = np.zeros(m, np.int32), leader.copy()
    if a.build_only:
        host_encode_lib()
        print(json.dumps(dict(messages=m, bytes=in_len, built=True)))
        return
    import torch  # the HIP runtime both sides share: before anything that loads libfpx.so

    from frankenpaxos_amd import wire

    host = host_encode_lib()

    lib = wire._L()
    per = (m + N - 1) // N
    cap = m * REPLY_MAX

    def locked(arr):
        p = C.c_void_p()
        assert lib.fpx_host_alloc(max(arr.nbytes, 8), C.byref(p)) == 0
        C.memmove(p, arr.ctypes.data, arr.nbytes)
        return p

    h_buf, h_off, h_to = locked(buf), locked(off), locked(to)
    stream = torch.cuda.Stream()
    hp = lambda v: C.c_void_p(v.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def fresh(direct=False):
        os.environ.pop("FPX_EPX_ENC_DIRECT", None)
        if direct:
            os.environ["FPX_EPX_ENC_DIRECT"] = "1"
        h = C.c_void_p()
        cfg = SIB.Cfg(N, SIB.DISTINCT, 0, 0, per)
        assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
        os.environ.pop("FPX_EPX_ENC_DIRECT", None)
        assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        assert lib.fpx_epx_keys_enable(h, 1 << 16) == 0
        return h

    i32a = lambda k: np.zeros(k, np.int32)
    soa_names = ("outcome", "ob", "os", "odeps", "oend", "otr")
    outs = lambda: dict(outcome=i32a(m), ob=i32a(m), os=i32a(m), odeps=i32a(m * N), oend=i32a(m), otr=i32a(m))
    out_args = lambda o: [hp(o[k]) for k in soa_names]
    rec_args = lambda o: [hp(x) for x in (to, leader, number, b_ord, b_rep, o["outcome"], o["ob"], o["os"], o["odeps"], o["oend"])]
    out1, off1 = np.zeros(cap, np.uint8), np.zeros(m + 1, np.int64)
    out2, off2, kind2, tot2 = np.zeros(cap, np.uint8), np.zeros(m + 1, np.int64), np.zeros(m, np.uint8), np.zeros(4, np.int64)
    t = {k: [] for k in ("1_tick_first", "1_encode_loop_first", "1_parent_path_first", "2_bytes_tick_first",
                         "2s_bytes_tick_with_soa_first", "1_tick_again", "1_encode_loop_again", "1_parent_path_again",
                         "2_bytes_tick_again", "2s_bytes_tick_with_soa_again", "3_encoder_span", "3_encoder_direct")}
    with torch.cuda.stream(stream):
        d_rec = [torch.from_numpy(x).cuda() for x in (to, leader, number, b_ord, b_rep)]
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        d_kind = torch.zeros(m, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    stream.synchronize()

    def timed_dev(fn, h):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert fn() == 0
        assert lib.fpx_epx_sync(h) == 0
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    need = encoded = 0
    for it in range(a.warmup + a.bursts):
        keep = it >= a.warmup
        # (1) the existing tick, then one encode call per message: on a fresh context (`first`: every message a PreAcceptOk; the
        # call also grows the context's buffers) and the same burst again (`again`: every message the PreAcceptOk again)
        h = fresh()
        o1 = outs()
        bad, npairs = C.c_int32(-9), C.c_int32(-9)
        ms1, ref = {}, {}
        for phase in ("first", "again"):
            t0 = time.perf_counter()
            st = lib.fpx_wire_epx_replica_tick(h, h_buf, in_len, h_off, m, h_to, 0, None, m, *out_args(o1), C.byref(bad), C.byref(npairs))
            t1 = time.perf_counter()
            cnt = C.c_int64(0)
            need = host.mb_encode_replies(N, m, *rec_args(o1), hp(out1), cap, hp(off1), C.byref(cnt))
            t2 = time.perf_counter()
            assert st == 0 and need > 0 and cnt.value == m, (st, need, cnt.value)
            assert np.isin(o1["outcome"], (1, 2)).all()            # a PreAcceptOk each, the first time or again
            ms1[phase] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            ref[phase] = (int(need), off1.copy(), out1[:need].copy(), {k: v.copy() for k, v in o1.items()})
        encoded = cnt.value
        assert lib.fpx_epx_destroy(h) == 0
        # (2) the bytes tick, nothing but the bytes asked for; (2s) with the six arrays as well
        res2 = {}
        for want_soa in (False, True):
            h = fresh()
            o2 = outs()
            for phase in ("first", "again"):
                t3 = time.perf_counter()
                st = lib.fpx_wire_epx_replica_tick_bytes(h, h_buf, in_len, h_off, m, h_to, 0, None, m, hp(out2), cap, hp(off2),
                                                         hp(kind2), hp(tot2), *(out_args(o2) if want_soa else [None] * 6),
                                                         C.byref(bad), C.byref(npairs))
                t4 = time.perf_counter()
                rn, roff, rout, rsoa = ref[phase]
                assert st == 0 and tot2.tolist() == [m, rn, 0, -1], (st, tot2.tolist())
                assert (off2 == roff).all() and (kind2 == 1).all() and out2[:rn].tobytes() == rout.tobytes()
                if want_soa:
                    assert all((rsoa[k] == o2[k]).all() for k in soa_names)
                res2[(want_soa, phase)] = (t4 - t3) * 1e3
            assert lib.fpx_epx_destroy(h) == 0
        # (3) the encoder alone on the tick's outputs in HBM, both forms
        ms3 = {}
        with torch.cuda.stream(stream):
            d_soa = [torch.from_numpy(ref["first"][3][k]).cuda() for k in ("outcome", "ob", "os", "odeps", "oend")]
        need, off1, out1f = ref["first"][0], ref["first"][1], ref["first"][2]
        stream.synchronize()
        for form in (("span", "direct") if it % 2 == 0 else ("direct", "span")):
            h = fresh(direct=form == "direct")
            call = lambda: lib.fpx_wire_epx_encode_replica_replies_dev(h, m, *[dp(x) for x in d_rec + d_soa], dp(d_out), cap, dp(d_off),
                                                                       dp(d_kind), dp(d_tot))
            timed_dev(call, h)                                   # (the scratch is sized, the code objects are loaded)
            d_out.zero_()
            stream.synchronize()
            ms3[form] = min(timed_dev(call, h) for _ in range(3))
            assert d_tot.tolist() == [m, need, 0, -1] and (d_off.cpu().numpy() == off1).all()
            assert d_out[:need].cpu().numpy().tobytes() == out1f.tobytes()
            assert lib.fpx_epx_destroy(h) == 0
        if keep:
            for phase in ("first", "again"):
                t["1_tick_" + phase].append(ms1[phase][0]), t["1_encode_loop_" + phase].append(ms1[phase][1])
                t["1_parent_path_" + phase].append(sum(ms1[phase]))
                t["2_bytes_tick_" + phase].append(res2[(False, phase)]), t["2s_bytes_tick_with_soa_" + phase].append(res2[(True, phase)])
            t["3_encoder_span"].append(ms3["span"]), t["3_encoder_direct"].append(ms3["direct"])
    out = dict(n=N, messages=m, in_bytes=in_len, reply_bytes=int(need), reply_bytes_per_message=round(need / m, 2), encoded=int(encoded),
               bursts=a.bursts)
    for k, v in t.items():
        med = statistics.median(v)
        out[k] = dict(ms_median=round(med, 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), msgs_per_s=round(m / med * 1e3))
    # (4) what comes down PCIe, and what the encoder moves in HBM
    out["4_copy_down_bytes"] = dict(parent_soa=(5 + N) * 4 * m + 8, bytes_tick=int(need) + 8 * (m + 1) + m + 32 + 8,
                                    bytes_tick_with_soa=int(need) + 8 * (m + 1) + m + 40 + (5 + N) * 4 * m)
    hbm_written = int(need) + 8 * (m + 1) + m
    hbm_read = 2 * (9 + N) * 4 * m                                 # the ten record arrays, read by the length pass and again by the emit pass
    for form in ("span", "direct"):
        ms = out["3_encoder_%s" % form]["ms_median"]
        out["3_encoder_%s" % form].update(hbm_bytes_written=hbm_written, hbm_bytes_read=hbm_read,
                                          gb_per_s=round((hbm_written + hbm_read) / ms / 1e6, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
