"""The acceptors' inbox as a reference proxy leader fills it: fpx_acceptor_inbox_dev against the same burst through the
parent commit's only route, fpx_acceptor_phase2a with single-bit target masks (the host call: the _dev form refuses a
burst that repeats a slot), and against multipaxos.Acceptor message at a time on one host thread
(acceptor_inbox_host.cpp).  The numbers of profiles/acceptor_inbox.md.

    python profiles/microbench/acceptor_inbox.py --mode inbox | inbox-mixed
    python profiles/microbench/acceptor_inbox.py --mode parent [--lib <libfpx.so of the PARENT commit>] [--slots N]
    python profiles/microbench/acceptor_inbox.py --mode inbox-mixed --dump burst.bin   (writes the burst for the host program)

The burst: --slots slots (default 2^20) x (f + 1) = 2 per-acceptor Phase2as at R = 3, f = 1, round 1 -- slot s goes to
acceptors s % 3 and (s + 1) % 3, the thrifty window of jni/Native.scala -- in arrival order: slot-major, shuffled inside
windows of 4096 messages.  inbox-mixed: 1 % of the messages are reads (MaxSlotRequest / BatchMaxSlotRequest) at random
positions and acceptors, and in the middle a leader change: three Phase1as of round 2 back to back, after which the
proxy leaders go on in round 1 for 3000 messages (Nacked) before they send round 2.
--mode parent uses only entry points the parent commit has, through plain ctypes, so that it runs on that commit's
library: the code under test is never its own yardstick.  It takes the Phase2as only (the parent has no call for the
others in a burst).  Every burst starts from fresh acceptors (fpx_reset, outside the timed region).  inbox: enqueue to
sync between two HIP events on the context's stream; parent: a host clock around the synchronous call.  The median of
--bursts runs after --warmup.  One JSON line.  Per-kernel times: run --mode inbox under rocprofv3 --kernel-trace --stats."""
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
PHASE2A, PHASE1A, MAX_SLOT_REQUEST, BATCH_MAX_SLOT_REQUEST = 1, 3, 10, 11
PHASE2B, NACK, PHASE1B = 2, 5, 9
R, WINDOW = 3, 4096


def make_burst(slots, mixed):
    rng = np.random.default_rng(1)
    s = np.repeat(np.arange(slots, dtype=np.int32), 2)
    a = ((s + np.tile(np.arange(2, dtype=np.int32), slots)) % R).astype(np.int32)
    order = np.arange(len(s))
    for lo in range(0, len(s), WINDOW):
        rng.shuffle(order[lo:lo + WINDOW])
    s, a = s[order], a[order]
    n2 = len(s)
    kind, rnd = np.full(n2, PHASE2A, np.int32), np.ones(n2, np.int32)
    value = (np.arange(n2, dtype=np.int64) * 2654435761 % (1 << 30)).astype(np.int32)
    if not mixed:
        return kind, a, s, rnd, value
    mid = n2 // 2
    rnd[mid + 3000:] = 2
    nreads = n2 // 100
    at = np.sort(np.concatenate([rng.integers(0, n2 + 1, nreads), np.full(3, mid)]))      # insertion points, Phase1as at mid
    is_p1a = np.zeros(len(at), bool)
    is_p1a[np.flatnonzero(at == mid)[:3]] = True
    ins_kind = np.where(is_p1a, PHASE1A, np.where(rng.random(len(at)) < 0.5, MAX_SLOT_REQUEST, BATCH_MAX_SLOT_REQUEST))
    ins_acc = np.where(is_p1a, np.cumsum(is_p1a) - 1, rng.integers(0, R, len(at)))
    ins = dict(kind=ins_kind, a=ins_acc, s=np.full(len(at), -1), rnd=np.where(is_p1a, 2, -1), value=np.full(len(at), -1))
    out = []
    for base, name in ((kind, "kind"), (a, "a"), (s, "s"), (rnd, "rnd"), (value, "value")):
        out.append(np.insert(base, at, ins[name].astype(np.int32)).astype(np.int32))
    return tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["inbox", "inbox-mixed", "parent"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"))
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dump", help="write the burst (n, slots, then kind, acceptor, slot, round, value as int32) here and exit")
    a = ap.parse_args()
    S = a.slots
    kind, acc, slot, rnd, value = make_burst(S, a.mode == "inbox-mixed")
    n = len(kind)
    if a.dump:
        with open(a.dump, "wb") as f:
            np.array([n, S], np.int32).tofile(f)
            for x in (kind, acc, slot, rnd, value):
                x.tofile(f)
        return
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd._lib import FpxConfig

    L = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
    cfg = FpxConfig(S, R, 1, 1, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
    h = C.c_void_p()
    assert L.fpx_create(C.byref(cfg), C.byref(h)) == 0
    hp = lambda x: C.c_void_p(x.ctypes.data)
    ms = []
    if a.mode == "parent":
        mask = np.zeros((n, 4), np.uint64)
        mask[np.arange(n), 0] = np.uint64(1) << acc.astype(np.uint64)
        votes, nacks = np.zeros((n, 4), np.uint64), np.zeros(n, np.int32)
        for it in range(a.warmup + a.bursts):
            assert L.fpx_reset(h) == 0 and L.fpx_sync(h) == 0
            t0 = time.perf_counter()
            assert L.fpx_acceptor_phase2a(h, n, hp(slot), hp(rnd), hp(value), hp(mask), hp(votes), None, hp(nacks)) == 0
            t1 = time.perf_counter()
            if it >= a.warmup:
                ms.append((t1 - t0) * 1e3)
        assert (votes == mask).all() and (nacks == -1).all()
        replies = dict(voted=int(n))
    else:
        stream = torch.cuda.Stream()
        assert L.fpx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        with torch.cuda.stream(stream):
            d = [torch.from_numpy(x).cuda() for x in (kind, acc, slot, rnd, value)]
            rk, rv = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        stream.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        for it in range(a.warmup + a.bursts):
            assert L.fpx_reset(h) == 0 and L.fpx_sync(h) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert L.fpx_acceptor_inbox_dev(h, n, p(d[0]), None, p(d[1]), p(d[2]), p(d[3]), p(d[4]), 0, p(rk), p(rv)) == 0
            assert L.fpx_sync(h) == 0
            e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        k = rk.cpu().numpy()
        replies = dict(voted=int((k == PHASE2B).sum()), nacked=int((k == NACK).sum()), promised=int((k == PHASE1B).sum()),
                       reads=int((k == MAX_SLOT_REQUEST).sum()))
        assert replies["voted"] + replies["nacked"] == int((kind == PHASE2A).sum())
        if a.mode == "inbox":
            assert replies["nacked"] == 0
        else:
            assert replies["promised"] == 3 and 0 < replies["nacked"] <= 3000
    pr, mv = np.zeros(R, np.int32), np.zeros(R, np.int32)
    assert L.fpx_read_scalars(h, hp(pr), hp(mv)) == 0
    assert mv.max() == S - 1 and pr.max() == (2 if a.mode == "inbox-mixed" else 1)
    digest = np.zeros(8, np.uint64)
    assert L.fpx_state_digest(h, hp(digest)) == 0
    print(json.dumps(dict(mode=a.mode, lib=os.path.abspath(a.lib), slots=S, messages=n, bursts=len(ms),
                          ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                          replies=replies, cells_digest="%016x%016x" % (int(digest[0]), int(digest[1])))))
    L.fpx_destroy(h)


if __name__ == "__main__":
    main()
