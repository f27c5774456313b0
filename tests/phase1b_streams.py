"""Bursts of Phase1b messages for fpx_leader_phase1b_msgs: the hand-written cases (their expected results worked out by
hand from Leader.handlePhase1b) and deterministic random streams.  tests/test_leader_phase1b_cpu.py holds the model of
tests/leader_phase1b_model.py to them without a GPU, tests/test_gpu_leader_phase1b.py the device.

A stream asserts its own promises (the run lengths it contains, where the quorum falls, how many records are walked),
so a change to a generator cannot quietly make a GPU test vacuous."""
import numpy as np

from tests.leader_phase1b_model import GRID, NOOP, Geometry, Msg, handle_burst

EDGE_RUNS = (0, 1, 63, 64, 65)     # the wavefront edges of a run, and no run at all
SEEDS = (1, 2, 3)                  # the seeds the tests run every shape with
UNIT = 256                         # records a wavefront walks (P1M_UNIT, fpx_phase1b_plan.hpp)


# ---- hand-written cases ---------------------------------------------------------------------------------------------
# name -> (config kwargs of the context, Geometry, call kwargs, messages, expected fields of the result)
def _r3(**kw):
    return dict(num_slots=64, num_replicas=3, f=1, **kw), Geometry(num_groups=kw.get("num_groups", 1),
                                                                  num_leader_groups=kw.get("num_leader_groups", 1), f=1, total=3)


A0 = Msg(4, 0, 0, [(2, 1, 10), (5, 3, 11)])
A1 = Msg(4, 0, 1, [(2, 2, 12)])
A2 = Msg(4, 0, 2, [(9, 1, 13)])
GRID22 = (dict(num_slots=64, num_replicas=4, quorum_kind=GRID, grid_rows=2, grid_cols=2),
          Geometry(total=4, quorum_kind=GRID, grid_rows=2, grid_cols=2))


def hand_cases():
    c = {}
    # (a) f = 1, one group, watermark 1: decides at A1; A2 never looked at
    c["a_basic"] = _r3() + (dict(round_=4, watermark=1), [A0, A1, A2],
                            dict(status=0, complete=1, decided_at=1, max_slot=5, next_slot=6, out_slot=[1, 2, 3, 4, 5],
                                 safe_round=[-1, 2, -1, -1, 3], safe_value=[NOOP, 12, NOOP, NOOP, 11], held={(0, 0), (0, 1)}))
    # (b) a stale-round message of A2 in between neither counts nor contributes
    c["b_stale"] = _r3() + (dict(round_=4, watermark=1), [A0, Msg(3, 0, 2, [(40, 9, 99)]), A1, A2],
                            dict(status=0, complete=1, decided_at=2, max_slot=5, next_slot=6,
                                 safe_value=[NOOP, 12, NOOP, NOOP, 11], held={(0, 0), (0, 1)}))
    # (c) a duplicate of A0 with other records: before k it replaces the first whole ...
    dup = Msg(4, 0, 0, [(3, 7, 70)])
    c["c_dup_before"] = _r3() + (dict(round_=4, watermark=1), [A0, dup, A1],
                                 dict(status=0, complete=1, decided_at=2, max_slot=3, next_slot=4, out_slot=[1, 2, 3],
                                      safe_round=[-1, 2, 7], safe_value=[NOOP, 12, 70]))
    # ... after k it does not
    c["c_dup_after"] = _r3() + (dict(round_=4, watermark=1), [A0, A1, dup],
                                dict(status=0, complete=1, decided_at=1, max_slot=5, safe_value=[NOOP, 12, NOOP, NOOP, 11]))
    # (d) two groups; group 0's third acceptor arrives before group 1's second: all three of group 0 are used
    g0 = [Msg(2, 0, a, [(4, a, 40 + a)]) for a in range(3)]
    g1 = [Msg(2, 1, 1, [(3, 1, 31)]), Msg(2, 1, 2, [(3, 2, 32), (7, 0, 72)])]
    c["d_two_groups"] = _r3(num_groups=2) + (dict(round_=2, watermark=0), [g0[0], g1[0], g0[1], g0[2], g1[1]],
                                             dict(status=0, complete=1, decided_at=4, max_slot=7, next_slot=8,
                                                  out_slot=list(range(8)), safe_round=[-1, -1, -1, 2, 2, -1, -1, 0],
                                                  safe_value=[NOOP, NOOP, NOOP, 32, 42, NOOP, NOOP, 72],
                                                  held={(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)}))
    # (e) nobody voted, watermark 7: literal nextSlot = maxSlot + 1 = 0
    c["e_no_votes"] = _r3() + (dict(round_=1, watermark=7), [Msg(1, 0, 2), Msg(1, 0, 0)],
                               dict(status=0, complete=1, decided_at=1, max_slot=-1, next_slot=0, count=0, out_slot=[]))
    # (f) no quorum yet (the second message is the same acceptor again)
    c["f_incomplete"] = _r3() + (dict(round_=4, watermark=1), [A0, dup], dict(status=0, complete=0, decided_at=-1))
    # (g) a Phase1b of a LARGER round: checkLt fires at its index, it is skipped, the others decide
    c["g_future"] = _r3() + (dict(round_=4, watermark=1), [A0, Msg(5, 0, 2, [(50, 5, 55)]), A1],
                             dict(status=9, err_index=1, complete=1, decided_at=2, max_slot=5, safe_value=[NOOP, 12, NOOP, NOOP, 11]))
    # (h) Mencius: L = 4, leader group 1, recoverSlot beyond every vote: slots 1, 5, 9, ...
    men = dict(num_slots=64, num_replicas=3, f=1, num_leader_groups=4), Geometry(num_leader_groups=4, f=1, total=3)
    m0, m1 = Msg(3, 0, 0, [(5, 1, 50), (9, 2, 90)]), Msg(3, 0, 2, [(5, 2, 52)])
    c["h_mencius"] = men + (dict(round_=3, watermark=3, leader_group=1, recover_slot=17), [m0, m1],
                            dict(status=0, complete=1, decided_at=1, max_slot=17, next_slot=21, out_slot=[5, 9, 13, 17],
                                 safe_round=[2, 2, -1, -1], safe_value=[52, 90, NOOP, NOOP], held={(1, 0), (1, 2)}))
    c["h_mencius_wm0"] = men + (dict(round_=3, watermark=0, leader_group=1, recover_slot=-1), [m0, m1],
                                dict(status=0, complete=1, max_slot=9, next_slot=13, out_slot=[1, 5, 9], safe_value=[NOOP, 52, 90]))
    c["h_mencius_not_owned"] = men + (dict(round_=3, watermark=3, leader_group=1, recover_slot=-1),
                                      [m0, Msg(3, 0, 2, [(5, 2, 52), (10, 1, 100)])],
                                      dict(status=9, err_index=-1, complete=None))
    # (i) a 2 x 2 grid: bits 0 1 / 2 3.  Row 0 complete after (0,0), (1,0), (0,1).  Slot 3 is row 1's by the literal rule:
    # only (1,0)'s record counts; with every row taken, (0,1)'s higher round wins
    gm = [Msg(1, 0, 0, [(2, 0, 20), (3, 1, 30)]), Msg(1, 1, 0, [(3, 2, 32)]), Msg(1, 0, 1, [(2, 4, 24), (3, 5, 35)])]
    c["i_grid_literal"] = GRID22 + (dict(round_=1, watermark=2, grid_cols=2), gm,
                                    dict(status=0, complete=1, decided_at=2, max_slot=3, out_slot=[2, 3], safe_round=[4, 2],
                                         safe_value=[24, 32], held={(0, 0), (0, 1), (0, 2)}))
    c["i_grid_all_rows"] = GRID22 + (dict(round_=1, watermark=2, grid_cols=2, all_rows=True), gm,
                                     dict(status=0, complete=1, decided_at=2, out_slot=[2, 3], safe_round=[4, 5], safe_value=[24, 35]))
    # (j) equal vote rounds at two acceptors with different values: the lower bit wins, whatever the order of arrival
    c["j_tie"] = _r3() + (dict(round_=4, watermark=0), [Msg(4, 0, 2, [(0, 3, 92)]), Msg(4, 0, 1, [(0, 3, 91)])],
                          dict(status=0, complete=1, out_slot=[0], safe_round=[3], safe_value=[91]))
    return c


def einval_cases():
    """(k) name -> (config kwargs, Geometry, call kwargs, messages, index, offsets_bad_at): every condition that makes
    a burst FPX_EINVAL, with the lowest offending index"""
    ok = Msg(4, 0, 1, [(2, 2, 12)])
    c = {}
    c["acceptor_high"] = _r3() + (dict(round_=4, watermark=0), [A0, Msg(4, 0, 3), ok, Msg(4, 0, 7)], 1, None)
    c["acceptor_negative"] = _r3() + (dict(round_=4, watermark=0), [Msg(4, 0, -1), A0, ok], 0, None)
    c["group_high"] = _r3() + (dict(round_=4, watermark=0), [A0, ok, Msg(4, 1, 0)], 2, None)
    c["group_negative"] = _r3() + (dict(round_=4, watermark=0), [A0, Msg(4, -2, 0), ok], 1, None)
    c["grid_column_high"] = GRID22 + (dict(round_=1, watermark=0, grid_cols=2), [Msg(1, 0, 0), Msg(1, 0, 2), Msg(1, 0, 1)], 1, None)
    c["grid_bit_high"] = GRID22 + (dict(round_=1, watermark=0, grid_cols=2), [Msg(1, 0, 0), Msg(1, 0, 1), Msg(1, 2, 0)], 2, None)
    c["vote_round_high"] = _r3() + (dict(round_=4, watermark=0), [A0, Msg(4, 0, 1, [(1, 2 ** 30 - 1, 5)])], 1, None)
    c["vote_round_negative"] = _r3() + (dict(round_=4, watermark=0), [Msg(4, 0, 0, [(1, 0, 5), (2, -1, 6)]), ok], 0, None)
    c["slots_equal"] = _r3() + (dict(round_=4, watermark=0), [A0, Msg(4, 0, 1, [(3, 1, 5), (3, 2, 6)])], 1, None)
    c["slots_descend"] = _r3() + (dict(round_=4, watermark=0), [Msg(4, 0, 2, [(6, 1, 5), (4, 2, 6), (8, 1, 1)]), ok], 0, None)
    c["slot_negative"] = _r3() + (dict(round_=4, watermark=0), [A0, Msg(4, 0, 1, [(-3, 1, 5)])], 1, None)
    c["offsets_descend"] = _r3() + (dict(round_=4, watermark=0), [A0, ok, A2], 1, 1)
    c["offsets_not_from_zero"] = _r3() + (dict(round_=4, watermark=0), [A0, ok], 0, 0)
    return c


def break_offsets(arrs, name):
    """the flat arrays of an offsets_* case, broken as the case says"""
    off = arrs["offsets"].copy()
    if name == "offsets_descend":
        off[2] = off[1] - 1          # message 1 ends before it starts
    else:
        off[0] = 1
    return dict(arrs, offsets=off)


# ---- random streams --------------------------------------------------------------------------------------------------
SHAPES = {
    # context kwargs; the stream's own knobs: acceptor groups, universe of slots (the call is stateless: record slots are
    # not bound by the context's window), flavour
    "r3_edges": dict(cfg=dict(num_slots=4096, num_replicas=3, f=2), U=4096, flavour="edges"),
    "r3_big": dict(cfg=dict(num_slots=4096, num_replicas=3, f=2), U=16384, flavour="big"),
    "r8_edges": dict(cfg=dict(num_slots=4096, num_replicas=8, f=5, num_groups=2), U=4096, flavour="edges"),
    "r8_big": dict(cfg=dict(num_slots=4096, num_replicas=8, f=3), U=16384, flavour="big"),
    "r130": dict(cfg=dict(num_slots=1024, num_replicas=130, f=69), U=1024, flavour="edges"),
}


class Stream:
    def __init__(self, shape, seed):
        sh = SHAPES[shape]
        cfg = sh["cfg"]
        rng = np.random.default_rng(seed)
        R, A, f, U = cfg["num_replicas"], cfg.get("num_groups", 1), cfg["f"], sh["U"]
        self.cfg = cfg
        self.geo = Geometry(num_groups=A, f=f, total=R)
        self.round, self.watermark = 6, U // 4 + 1
        order = [(g, a) for g in range(A) for a in range(R)]
        order = [order[i] for i in rng.permutation(len(order))]
        msgs = []
        for j, (g, a) in enumerate(order):
            mine = np.arange(g, U, A)                      # the slots of the acceptor's group
            if sh["flavour"] == "big":
                n = int(0.6 * len(mine))
            else:
                n = EDGE_RUNS[(j + seed) % len(EDGE_RUNS)] if j < 2 * len(EDGE_RUNS) else int(rng.integers(0, max(8, 3 * len(mine) // (f + 1))))
            n = min(n, len(mine))
            slots = np.sort(rng.choice(mine, size=n, replace=False))
            if n > 2:                                      # a slot of another group: never looked up by the handler
                slots[n // 2] = slots[n // 2] + 1 if A > 1 and slots[n // 2] + 1 < slots[n // 2 + 1] else slots[n // 2]
            info = [(int(s), int(rng.integers(0, 4)), int(rng.integers(0, 1000))) for s in slots]
            msgs.append(Msg(self.round, g, a, info))
            if j == 1:                                     # a stale answer, a foreign kind, and a replacement of the first
                msgs.append(Msg(self.round - 1, g, a, [(5, 5, 5)]))
                msgs.append(Msg(self.round, g, a, [(1, 1, 1)], kind=2))
                first = msgs[0]
                msgs.append(Msg(self.round, first.group, first.acceptor, [(s + A, r, v + 1) for s, r, v in first.info[::2] if s + A < U]))
        self.msgs = msgs
        self.want = handle_burst(self.geo, self.round, self.watermark, msgs)
        if self.want.count % 64 == 0:                     # (not a whole number of wavefronts of entries)
            self.watermark += 1
            self.want = handle_burst(self.geo, self.round, self.watermark, msgs)
        # ---- promises
        w = self.want
        assert w.status == 0 and w.complete == 1 and w.count % 64 != 0 and w.count > 64
        assert 3 < w.decided_at < len(msgs) - 1 or A * (f + 1) >= len(order) - 1, "messages before and after the decision"
        used = [m for m in msgs[: w.decided_at + 1] if m.kind == 9 and m.round == self.round]
        lens = {len(m.info) for m in used}
        self.walked = sum(len(m.info) for m in used)
        self.used_runs = lens                             # (R = 3 holds three of EDGE_RUNS per seed: the seeds together hold all)
        if sh["flavour"] == "edges":
            assert lens >= set(EDGE_RUNS) or R < 5, lens
        else:
            assert self.walked > 20000 and max(lens) > 4 * UNIT * 4, "runs that straddle workgroups"
        assert any(sr >= 0 for sr in w.safe_round) and any(sr < 0 for sr in w.safe_round)
