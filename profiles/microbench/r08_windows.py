"""the headline step (2^20 fresh slots x 256 acceptors, PER_SLOT, fused, device pointers, round 0), one launch per log
window, with the vote kernel's time of EVERY launch (fpx_profile_read_launches) printed beside its window.  Set against
the placement probe of the same windows (FPX_DEBUG=1 prints it when the context is created) this is the kernel's
distance from its windows' pair ceiling (profiles/r08_steady_walk.md).  Imports frankenpaxos_amd from the current
directory.  AB_WINDOWS: log windows (the first AB_WARM of them are the warm-up and are not timed)"""
import json, os, sys
sys.path.insert(0, os.getcwd())
import torch
import frankenpaxos_amd as fa

N = 1 << 20
WIN = int(os.environ.get("AB_WINDOWS", "16"))
WARM = int(os.environ.get("AB_WARM", "2"))
dev = torch.device("cuda:0")
ctx = fa.Context(fa.make_config(num_slots=WIN * N, num_replicas=256, f=127, quorum_kind=fa.FPX_Q_THRESHOLD,
                                ballot_mode=fa.FPX_BALLOT_PER_SLOT, tally_ways=4, device=0, flags=fa.FPX_F_TRUSTED))
stream = torch.cuda.current_stream()
ctx.set_stream(stream.cuda_stream)
assert ctx.acceptor_phase1a(0, 0)[0] == 0
ctx.flush_promises()
steps = []
for w in range(WIN):
    slot = torch.arange(w * N, (w + 1) * N, dtype=torch.int32, device=dev)
    steps.append((slot, torch.zeros(N, dtype=torch.int32, device=dev), (slot * 7 + 3).to(torch.int32),
                  torch.zeros(N, dtype=torch.uint8, device=dev), torch.full((N,), -7, dtype=torch.int32, device=dev),
                  torch.full((N,), -7, dtype=torch.int32, device=dev)))
def step(w):
    s, r, v, ch, cr, cv = steps[w]
    ctx.phase2_fused_dev(s, r, v, None, ch, cr, cv)
for w in range(WARM):
    step(w)
assert ctx.sync() == 0
torch.cuda.synchronize()
ctx.profile_enable(True)
for w in range(WARM, WIN):
    step(w)
torch.cuda.synchronize()
per = ctx.profile_read_launches()
assert ctx.sync() == 0 and len(per) == WIN - WARM, (len(per), WIN - WARM)
for w in range(WARM, WIN):
    s, r, v, ch, cr, cv = steps[w]
    assert bool(ch.all()) and bool((cv == v).all()) and bool((cr == 0).all()), "window %d not all chosen" % w
out = {"kernel_ms": {w: float(per[w - WARM]) for w in range(WARM, WIN)}}
out["mean_ms"] = sum(per) / len(per)
if hasattr(ctx, "ballot_summary_audit"):
    out["audit"] = ctx.ballot_summary_audit()
print(json.dumps(out), flush=True)
ctx.close()
