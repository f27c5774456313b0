"""A Mencius acceptor's inbox as reference proxy leaders fill it: fpx_mencius_acceptor_inbox_dev against the same burst through
the parent commit's only route (the HOST calls fpx_acceptor_phase2a and fpx_acceptor_phase2a_noop_ranges with single-bit
target masks) and against mencius.Acceptor message at a time on one host thread (mencius_acceptor_inbox_host.cpp).  The
numbers of profiles/mencius_acceptor_inbox.md.

    python profiles/microbench/mencius_acceptor_inbox.py --mode inbox [--ranges-per-acceptor 1 | 8 | 64]
    python profiles/microbench/mencius_acceptor_inbox.py --mode parent --fraction 8 [--lib <libfpx.so of the PARENT commit>]
    python profiles/microbench/mencius_acceptor_inbox.py --mode inbox --dump burst.bin   (writes the burst for the host program)

The burst, on a context shaped like BASELINE.json configs[4] (256 leader groups, one acceptor group of R = 3, f = 1) with
2^21 slots, 8192 rows per leader group: the 128 even leader groups propose -- each of their 2^20 slots arrives as
quorumSize = 2 per-acceptor Phase2as, slot s to acceptors q % 3 and (q + 1) % 3 of its group (q = s / 256), 2^21 messages
-- and the 128 odd ones skip: --ranges-per-acceptor k Phase2aNoopRanges per acceptor address to 2 acceptors of the group,
the group's 8192 rows cut into k consecutive ranges, 256 k messages, all in round 1.  Arrival order: slot-major with
every range where its start falls, shuffled inside windows of 4096 messages.
--mode parent uses only entry points the parent commit has, through plain ctypes, so that it runs on that commit's
library: the code under test is never its own yardstick.  --fraction F takes the first 1/F of the burst's Phase2as and
of its ranges (the host route is 0.1 ms per thousand messages); the JSON line says how many messages ran.  Every burst
starts from fresh acceptors (fpx_reset, outside the timed region).  inbox: enqueue to sync between two HIP events on the
context's stream; parent: a host clock around the two synchronous calls.  The median of --bursts runs after --warmup.
One JSON line.  Per-kernel times: run --mode inbox under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PHASE2A, PHASE2A_NOOP_RANGE = 1, 6
PHASE2B, PHASE2B_NOOP_RANGE, NACK = 2, 7, 5
L, A, R, WINDOW = 256, 1, 3, 4096


def make_burst(S, k):
    """-> kind, group, acceptor, slot, slot_end, round, value (int32 each)"""
    rng = np.random.default_rng(1)
    rows = S // L
    s = np.arange(S, dtype=np.int64)
    s = s[(s % L) % 2 == 0]                                   # the proposing leader groups' slots, in slot order
    s = np.repeat(s, 2)
    q = s // L
    a = (q + np.tile(np.arange(2), len(s) // 2)) % R
    kind, end = np.full(len(s), PHASE2A), np.full(len(s), -1)
    # the ranges: leader group lg (odd), rows [j rows / k, (j + 1) rows / k), to acceptors j % 3 and (j + 1) % 3
    lg = np.repeat(np.arange(1, L, 2), k * 2)
    j = np.tile(np.repeat(np.arange(k), 2), L // 2)
    r0, r1 = j * rows // k, (j + 1) * rows // k
    rs, re = r0 * L + lg, (r1 - 1) * L + lg + 1
    ra = (j + np.tile(np.arange(2), len(lg) // 2)) % R
    at = np.searchsorted(s, rs)                               # where the start falls in slot order
    kind = np.insert(kind, at, PHASE2A_NOOP_RANGE)
    slot, end = np.insert(s, at, rs), np.insert(end, at, re)
    acc = np.insert(a, at, ra)
    group = slot % L                                          # A = 1: the context's row of the leader group
    n = len(kind)
    order = np.arange(n)
    for lo in range(0, n, WINDOW):
        rng.shuffle(order[lo:lo + WINDOW])
    value = np.where(kind == PHASE2A, np.arange(n, dtype=np.int64) * 2654435761 % (1 << 30), -1)
    out = [x[order].astype(np.int32) for x in (kind, group, acc, slot, end)]
    return out + [np.ones(n, np.int32), value[order].astype(np.int32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["inbox", "parent"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"))
    ap.add_argument("--slots", type=int, default=1 << 21)
    ap.add_argument("--ranges-per-acceptor", type=int, default=1)
    ap.add_argument("--fraction", type=int, default=1)
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dump", help="write the burst (n, S, L, A, R, then the seven int32 arrays) here and exit")
    a = ap.parse_args()
    S = a.slots
    assert S % (2 * L) == 0
    kind, group, acc, slot, end, rnd, value = make_burst(S, a.ranges_per_acceptor)
    n = len(kind)
    if a.dump:
        with open(a.dump, "wb") as f:
            np.array([n, S, L, A, R], np.int32).tofile(f)
            for x in (kind, group, acc, slot, end, rnd, value):
                x.tofile(f)
        return
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd._lib import FpxConfig

    lib = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
    cfg = FpxConfig(S, R, A, L, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
    h = C.c_void_p()
    assert lib.fpx_create(C.byref(cfg), C.byref(h)) == 0
    hp = lambda x: C.c_void_p(x.ctypes.data)
    ms = []
    if a.mode == "parent":
        p2a, nr = np.flatnonzero(kind == PHASE2A), np.flatnonzero(kind == PHASE2A_NOOP_RANGE)
        p2a, nr = p2a[:len(p2a) // a.fraction], nr[:max(1, len(nr) // a.fraction)]
        n = len(p2a) + len(nr)
        ps, pr, pv = (np.ascontiguousarray(x[p2a]) for x in (slot, rnd, value))
        pm = np.zeros((len(p2a), 4), np.uint64)
        pm[:, 0] = np.uint64(1) << acc[p2a].astype(np.uint64)
        rs, re, rr = (np.ascontiguousarray(x[nr]) for x in (slot, end, rnd))
        rm = np.zeros((len(nr), A, 4), np.uint64)
        rm[:, 0, 0] = np.uint64(1) << acc[nr].astype(np.uint64)
        pvotes, pnacks = np.zeros((len(p2a), 4), np.uint64), np.zeros(len(p2a), np.int32)
        rvotes, rnacks, rnr = np.zeros((len(nr), A, 4), np.uint64), np.zeros((len(nr), A, 4), np.uint64), np.zeros(len(nr), np.int32)
        for it in range(a.warmup + a.bursts):
            assert lib.fpx_reset(h) == 0 and lib.fpx_sync(h) == 0
            t0 = time.perf_counter()
            assert lib.fpx_acceptor_phase2a(h, len(p2a), hp(ps), hp(pr), hp(pv), hp(pm), hp(pvotes), None, hp(pnacks)) == 0
            assert lib.fpx_acceptor_phase2a_noop_ranges(h, len(nr), hp(rs), hp(re), hp(rr), hp(rm), hp(rvotes), hp(rnacks),
                                                        hp(rnr)) == 0
            t1 = time.perf_counter()
            if it >= a.warmup:
                ms.append((t1 - t0) * 1e3)
        assert (pvotes == pm).all() and (pnacks == -1).all() and (rvotes == rm).all() and not rnacks.any()
        replies = dict(voted=int(len(p2a)), voted_ranges=int(len(nr)))
    else:
        stream = torch.cuda.Stream()
        assert lib.fpx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        with torch.cuda.stream(stream):
            d = [torch.from_numpy(x).cuda() for x in (kind, group, acc, slot, end, rnd, value)]
            rk, rv = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        stream.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        for it in range(a.warmup + a.bursts):
            assert lib.fpx_reset(h) == 0 and lib.fpx_sync(h) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert lib.fpx_mencius_acceptor_inbox_dev(h, n, *(p(t) for t in d), p(rk), p(rv)) == 0
            assert lib.fpx_sync(h) == 0
            e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        k = rk.cpu().numpy()
        replies = dict(voted=int((k == PHASE2B).sum()), voted_ranges=int((k == PHASE2B_NOOP_RANGE).sum()),
                       nacked=int((k == NACK).sum()))
        assert replies["voted"] == S and replies["voted_ranges"] == L * a.ranges_per_acceptor and replies["nacked"] == 0
        vr, vv, bl = (np.zeros((S, R), np.int32) for _ in range(3))    # (named: the call writes all three)
        assert lib.fpx_read_state(h, hp(vr), hp(vv), hp(bl)) == 0
        assert ((vr == 1).sum(axis=1) == 2).all()            # every slot of the band holds two votes
    pr, mv = np.zeros((L, R), np.int32), np.zeros((L, R), np.int32)
    assert lib.fpx_read_scalars(h, hp(pr), hp(mv)) == 0
    assert pr.max() == 1 and (a.fraction > 1 or mv.max() == S - 1)
    digest = np.zeros(8, np.uint64)
    assert lib.fpx_state_digest(h, hp(digest)) == 0
    print(json.dumps(dict(mode=a.mode, lib=os.path.abspath(a.lib), slots=S, ranges_per_acceptor=a.ranges_per_acceptor,
                          fraction=a.fraction, messages=n, bursts=len(ms), ms_median=round(statistics.median(ms), 4),
                          ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), replies=replies,
                          cells_digest="%016x%016x" % (int(digest[0]), int(digest[1])))))
    lib.fpx_destroy(h)


if __name__ == "__main__":
    main()
