"""A leader change at every acceptor: the batched Phase1b.info pass against the per-acceptor loop.

Setting (--shape headline): a 2^20 x 256 context with a ballot per cell, the lower half of the window voted by every
acceptor, the upper half by a thrifty run of f + 1 acceptors, watermark S / 4.  --shape cfg5: 256 leader groups x 3
acceptors, one leader group addressed.  3 warm-ups, median of --reps (default 20):

  (a) fpx_acceptor_phase1b_info_all_dev, timed with events on the context's stream, and its algorithmic bytes (one
      read of the two vote arrays from the watermark on, plus the records written) per second
  (b) fpx_acceptor_phase1 on host arrays, end to end (wall clock)
  (c) the loop it replaces: per addressed acceptor fpx_acceptor_phase1a with one bit + fpx_acceptor_phase1b_info
      (sized call + filled call, as the bindings do), wall clock -- untouched code, the parent's figure

Prints one JSON line (profiles/phase1_info.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import frankenpaxos_amd as fa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["headline", "cfg5"], default="headline")
ap.add_argument("--log-slots", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--loop-reps", type=int, default=20)
args = ap.parse_args()
WARM = 3
S = 1 << args.log_slots
dev = torch.device("cuda:0")

if args.shape == "headline":
    R, L = 256, 1
    cfg = fa.make_config(num_slots=S, num_replicas=R, f=127, ballot_mode=1)
else:
    R, L = 3, 256
    cfg = fa.make_config(num_slots=S, num_replicas=R, f=1, num_leader_groups=L, ballot_mode=1)
ctx = fa.Context(cfg)
ng, E, wm = L, L * R, S // 4
f1 = cfg.f + 1

# the votes: everybody in the lower half, a thrifty run of f + 1 acceptors in the upper half
slot = torch.arange(S, dtype=torch.int32, device=dev)
rnd = torch.zeros(S, dtype=torch.int32, device=dev)
tgt = np.zeros((S, 4), np.uint64)
run = np.zeros(256, bool)
run[:f1] = True
full = np.zeros(256, bool)
full[:R] = True
for w in range(4):
    bits = lambda m: sum(1 << k for k in range(64) if m[64 * w + k])
    tgt[: S // 2, w] = np.uint64(bits(full))
    tgt[S // 2:, w] = np.uint64(bits(run))
ttgt = torch.from_numpy(tgt.view(np.int64)).to(dev)
ch = torch.zeros(S, dtype=torch.uint8, device=dev)
cr, cv = torch.zeros_like(slot), torch.zeros_like(slot)
ctx.phase2_fused_dev(slot, rnd, slot, ttgt, ch, cr, cv)
assert ctx.sync() == 0

masks = None
addressed = [(g, r) for g in range(ng) for r in range(R)]
if args.shape == "cfg5":
    masks = np.zeros((ng, 4), np.uint64)
    masks[0, 0] = np.uint64((1 << R) - 1)
    addressed = [(0, r) for r in range(R)]
tmask = None if masks is None else torch.from_numpy(masks.view(np.int64)).to(dev)

# sizing
off, sl, vr, vv = ctx.acceptor_phase1b_info_all(wm, masks)
total = int(off[-1])
rows = (S - wm) if args.shape == "headline" else (S - wm) // L
algo_bytes = 2 * rows * 4 * ((R + 3) & ~3) + 12 * total

# (a)
d_off = torch.zeros(E + 1, dtype=torch.int64, device=dev)
d_rec = [torch.zeros(max(total, 1), dtype=torch.int32, device=dev) for _ in range(3)]
d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
stream = torch.cuda.Stream(device=dev)
ctx.set_stream(stream.cuda_stream)
ta = []
for rep in range(WARM + args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.acceptor_phase1b_info_all_dev(wm, tmask, total, d_off, d_rec[0], d_rec[1], d_rec[2], d_tot)
    e1.record(stream)
    e1.synchronize()
    if rep >= WARM:
        ta.append(e0.elapsed_time(e1))
assert ctx.sync() == 0 and d_tot.tolist() == [total, total]
assert np.array_equal(d_rec[0].cpu().numpy()[:total], sl) and np.array_equal(d_off.cpu().numpy(), off)
ctx.set_stream(None)

# (b)
pb, nb = np.zeros((ng, 4), np.uint64), np.zeros((ng, 4), np.uint64)
k = C.c_int64()
hp = lambda a: None if a is None else a.ctypes.data
tb, rnd_next = [], 1
for rep in range(WARM + args.reps):
    t0 = time.perf_counter()
    st = ctx.L.fpx_acceptor_phase1(ctx._h, rnd_next, wm, hp(masks), hp(pb), hp(nb), total, hp(off), hp(sl), hp(vr), hp(vv), C.byref(k))
    t1 = time.perf_counter()
    assert st == 0 and k.value == total, (st, k.value)
    rnd_next += 1
    if rep >= WARM:
        tb.append((t1 - t0) * 1e3)

# (c)
tc, got = [], 0
for rep in range(WARM + args.loop_reps):
    t0 = time.perf_counter()
    got = 0
    for g, r in addressed:
        one = np.zeros(4, np.uint64)
        one[r >> 6] = np.uint64(1 << (r & 63))
        st, p, n_ = ctx.acceptor_phase1a(g, rnd_next, wm, one)
        assert st == 0 and p.any()
        got += len(ctx.acceptor_phase1b_info(g, r, wm)[0])
    t1 = time.perf_counter()
    rnd_next += 1
    if rep >= WARM:
        tc.append((t1 - t0) * 1e3)
assert got == total, (got, total)

med = lambda x: float(np.median(x))
print(json.dumps(dict(shape=args.shape, slots=S, replicas=R, leader_groups=L, watermark=wm, acceptors_addressed=len(addressed),
                      records=total, algorithmic_bytes=algo_bytes,
                      a_dev_ms_median=med(ta), a_dev_ms_min=float(min(ta)), a_algorithmic_GBps=algo_bytes / med(ta) / 1e6,
                      b_host_ms_median=med(tb), b_host_ms_min=float(min(tb)),
                      c_loop_ms_median=med(tc), c_loop_ms_min=float(min(tc)),
                      ratio_c_over_b=med(tc) / med(tb), ratio_c_over_a=med(tc) / med(ta), reps=args.reps, loop_reps=args.loop_reps)))
ctx.close()
