"""One tick of a Mencius proxy leader among remote acceptors at BASELINE config 5's shape (L = 256 leader groups, A = 1,
R = 3, f = 1, S = 2^22), device time of the tally only (the arrays are resident; host clock around call + fpx_sync):

  --burst cfg5          2^20 Phase2b's (2^19 slots x 2 votes, slot-major) with the Phase2bNoopRanges of 256 ranges (2 or 3
                        votes each) interleaved at random positions
  --burst phase2b_only  the same 2^20 Phase2b's, no range message

  --call mencius   fpx_mencius_proxy_phase2b_msgs_dev on the whole burst (kind = NULL for phase2b_only)
  --call parent    the route of the commit before: fpx_proxy_phase2b_msgs_dev on the same arrays (it skips the range
                   messages), and for cfg5 a one-thread host fold of the range messages into rows (numpy) +
                   fpx_proxy_phase2b_noop_ranges.  --lib picks the library (a build of that commit), so the new code is
                   never its own yardstick.

Prints one JSON line: ms per call (median, min, 10th / 90th percentile, all) after --warmup calls; every repetition
starts from a reset context with the same opens, and the outputs are checked.  Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel times (profiles/mencius_phase2b_msgs.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--burst", choices=["cfg5", "phase2b_only"], required=True)
ap.add_argument("--call", choices=["mencius", "parent"], required=True)
ap.add_argument("--lib", default=None)
ap.add_argument("--log-msgs", type=int, default=20)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402

from frankenpaxos_amd._lib import FpxConfig  # noqa: E402

PHASE2B, RANGE = 2, 7
Lg, A, R, f, S = 256, 1, 3, 1, 1 << 22
VP, I32 = C.c_void_p, C.c_int32
rng = np.random.default_rng(1)

# ---- the burst ---------------------------------------------------------------------------------------------------------
nslots = 1 << (args.log_msgs - 1)
p_slot = np.repeat(np.arange(nslots, dtype=np.int32), 2)
p_acc = rng.permuted(np.tile(np.arange(R, dtype=np.int32), (nslots, 1)), axis=1)[:, :2].reshape(-1)  # two DIFFERENT acceptors
r_start = ((1 << 21) + np.arange(Lg)).astype(np.int32)                  # one range per leader group, above the commands
r_end = (r_start + Lg * rng.integers(1, 64, size=Lg)).astype(np.int32)
votes = rng.integers(2, 4, size=Lg)                                      # 2 or 3 votes: every range completes
r_ent = np.repeat(np.arange(Lg), votes)
r_acc = np.concatenate([rng.permutation(R)[:k] for k in votes]).astype(np.int32)
if args.burst == "phase2b_only":
    r_ent, r_acc = r_ent[:0], r_acc[:0]
n = len(p_slot) + len(r_ent)
is_range = np.zeros(n, bool)
is_range[rng.choice(n, size=len(r_ent), replace=False)] = True
kind = np.where(is_range, RANGE, PHASE2B).astype(np.int32)
slot, end, acc = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
slot[~is_range], acc[~is_range] = p_slot, p_acc
slot[is_range], end[is_range], acc[is_range] = r_start[r_ent], r_end[r_ent], r_acc
rnd, grp = np.zeros(n, np.int32), np.zeros(n, np.int32)

lib = C.CDLL(os.path.abspath(args.lib) if args.lib else os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"),
             mode=C.RTLD_GLOBAL)
cfg = FpxConfig(S, R, A, Lg, f, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
h = VP()
assert lib.fpx_create(C.byref(cfg), C.byref(h)) == 0
dev = torch.device("cuda:0")
d = {k: torch.from_numpy(v).to(dev) for k, v in dict(kind=kind, grp=grp, acc=acc, slot=slot, end=end, rnd=rnd).items()}
ch = torch.zeros(n, dtype=torch.uint8, device=dev)
cr = torch.zeros(n, dtype=torch.int32, device=dev)
cv = torch.zeros(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
open_slot, zeros = np.arange(nslots, dtype=np.int32), np.zeros(nslots, np.int32)
vals, new = np.arange(nslots, dtype=np.int32), np.zeros(nslots, np.uint8)
r_round, r_new = np.zeros(Lg, np.int32), np.zeros(Lg, np.uint8)


def ptr(a):
    return VP(a.ctypes.data)


def dp(t):
    return VP(t.data_ptr())


def reopen():
    assert lib.fpx_reset(h) == 0
    assert lib.fpx_proxy_open(h, I32(nslots), ptr(open_slot), ptr(zeros), ptr(vals), ptr(new)) == 0
    assert lib.fpx_proxy_open_noop_ranges(h, I32(Lg), ptr(r_start), ptr(r_end), ptr(r_round), ptr(r_new)) == 0
    assert lib.fpx_sync(h) == 0


def fold_ranges():
    """the range messages of the burst as rows, in order of first appearance: one thread on the host"""
    at = np.nonzero(kind == RANGE)[0]
    keys = slot[at].astype(np.int64) << 32 | end[at].astype(np.int64)     # (one round in this burst)
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    rows = np.zeros((len(uniq), A, 4), np.uint64)
    np.bitwise_or.at(rows, (rank[inv], grp[at], acc[at] >> 6), np.uint64(1) << (acc[at] & 63).astype(np.uint64))
    f0 = at[first[order]]
    return slot[f0].copy(), end[f0].copy(), rnd[f0].copy(), rows


times, fold_ms, chosen_ranges = [], [], 0
for rep in range(args.warmup + args.reps):
    reopen()
    t0 = time.perf_counter()
    if args.call == "mencius":
        st = lib.fpx_mencius_proxy_phase2b_msgs_dev(h, I32(n), dp(d["kind"]) if len(r_ent) else None, dp(d["grp"]), dp(d["acc"]),
                                                    dp(d["slot"]), dp(d["end"]), dp(d["rnd"]), dp(ch), dp(cr), dp(cv))
        assert st == 0 and lib.fpx_sync(h) == 0
        t1 = time.perf_counter()
    else:
        st = lib.fpx_proxy_phase2b_msgs_dev(h, I32(n), dp(d["kind"]) if len(r_ent) else None, None, dp(d["acc"]), dp(d["slot"]),
                                            dp(d["rnd"]), I32(0), dp(ch), dp(cr), dp(cv))
        assert st == 0 and lib.fpx_sync(h) == 0
        tf = time.perf_counter()
        if len(r_ent):
            fs, fe, fr, rows = fold_ranges()
            tg = time.perf_counter()
            rch = np.zeros(len(fs), np.uint8)
            assert lib.fpx_proxy_phase2b_noop_ranges(h, I32(len(fs)), ptr(fs), ptr(fe), ptr(fr), ptr(rows), ptr(rch)) == 0
            chosen_ranges = int(rch.sum())
            if rep >= args.warmup:
                fold_ms.append((tg - tf) * 1e3)
        t1 = time.perf_counter()
    if rep >= args.warmup:
        times.append((t1 - t0) * 1e3)
    flags = ch.cpu().numpy()
    if args.call == "mencius":
        chosen_ranges = int(flags[is_range].sum())
    # two votes of three acceptors, f = 1: every slot is chosen, at its first message; and every range
    assert int(flags[~is_range].sum()) == nslots and chosen_ranges == (Lg if len(r_ent) else 0), (flags.sum(), chosen_ranges)
t = np.array(times)
res = dict(burst=args.burst, call=args.call, lib=args.lib or "tree", messages=n, range_messages=int(len(r_ent)), reps=len(times),
           ms_median=float(np.median(t)), ms_min=float(t.min()), ms_p10=float(np.percentile(t, 10)),
           ms_p90=float(np.percentile(t, 90)), ms_all=[round(x, 4) for x in times])
if fold_ms:
    res["ms_host_fold_median"] = float(np.median(fold_ms))
print(json.dumps(res))
lib.fpx_destroy(h)
