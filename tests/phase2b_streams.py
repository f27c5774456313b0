"""Streams of per-acceptor Phase2b messages for fpx_proxy_phase2b_msgs (tests/test_gpu_phase2b_msgs.py runs them on the
GPU, tests/test_phase2b_msgs_cpu.py checks on the oracle alone that they are not vacuous).

A stream opens a set of (slot, round) entries and gives every entry the votes of a random subset of its acceptors, of a
size uniform in 0 .. R (so about half of the entries reach a majority-sized quorum and the others stay Pending), with
10 % of the votes sent twice; the messages are laid out slot-major (the votes of an entry adjacent), acceptor-major, or
in a random permutation, and cut to exactly n messages."""
import numpy as np

GRID = 2  # FPX_Q_GRID

# the smallest shapes at which each code path can go wrong
SHAPES = {
    "r3": dict(num_slots=4096, num_replicas=3, f=1),                                    # baseline threshold quorum
    "ways4": dict(num_slots=4096, num_replicas=5, f=2, tally_ways=4),                   # several ways per slot
    "grid2x3": dict(num_slots=4096, num_replicas=6, quorum_kind=GRID, grid_rows=2, grid_cols=3),  # group_index matters
    "r256": dict(num_slots=512, num_replicas=256, f=127),                               # bits in all four words
    "lg4": dict(num_slots=4096, num_replicas=3, f=1, num_leader_groups=4),              # leader-group-major rows
}
LAYOUTS = ("slot_major", "acceptor_major", "random")
LENGTHS = (1, 63, 64, 65, 257, 20000)  # the wavefront and workgroup edges; many workgroups
PHASE2B = 2  # FPX_WIRE_PHASE2B


class Stream:
    """open_slot / open_round / open_value: the entries to open; group_index / acceptor_index / slot / round: the n
    messages; grid_cols: what the entry points take (0 unless the shape is a grid); bit: the acceptor bit per message"""

    def __init__(self, shape, n, layout, seed):
        kw = SHAPES[shape]
        rng = np.random.default_rng(seed)
        S, R = kw["num_slots"], kw["num_replicas"]
        self.kw, self.grid_cols = kw, kw.get("grid_cols", 0)
        two_rounds = shape == "ways4"
        entries = max(1, int(np.ceil(n / (0.55 * R)))) + 2
        while True:
            # entry e = (slots[e % nslots], round e // nslots): further rounds of the same slots once the window's slots
            # are used up (every shape keeps 4 tallies per slot), and two rounds of half the slots in any case when the
            # shape is about the ways
            entries = min(entries, 4 * S)
            nslots = min(S, int(np.ceil(entries / 1.5)) if two_rounds else entries)
            slots = rng.choice(S, size=nslots, replace=False).astype(np.int32)
            oslot = [int(slots[e % nslots]) for e in range(entries)]
            oround = [e // nslots for e in range(entries)]
            ent, bit = [], []
            for e in range(len(oslot)):
                k = int(rng.integers(0, R + 1))
                for b in rng.choice(R, size=k, replace=False):
                    ent.append(e), bit.append(int(b))
            ent, bit = np.array(ent, np.int64), np.array(bit, np.int64)
            dup = rng.random(len(ent)) < 0.10
            ent, bit = np.concatenate([ent, ent[dup]]), np.concatenate([bit, bit[dup]])
            if len(ent) >= n or entries == 4 * S:
                break
            entries = entries + max(2, entries // 10)
        if layout == "slot_major":
            order = np.argsort(ent, kind="stable")
        elif layout == "acceptor_major":
            order = np.argsort(bit, kind="stable")
        else:
            order = rng.permutation(len(ent))
        order = order[:n]
        ent, bit = ent[order], bit[order]
        self.open_slot = np.array(oslot, np.int32)
        self.open_round = np.array(oround, np.int32)
        self.open_value = (1000 + np.arange(len(oslot))).astype(np.int32)
        self.bit = bit.astype(np.int32)
        self.slot = self.open_slot[ent]
        self.round = self.open_round[ent]
        if self.grid_cols:
            self.group_index = (bit // self.grid_cols).astype(np.int32)
            self.acceptor_index = (bit % self.grid_cols).astype(np.int32)
        else:
            self.group_index = np.zeros(len(bit), np.int32)
            self.acceptor_index = bit.astype(np.int32)
        self.n = len(bit)

    def decoded(self, lo=0, hi=None):
        """messages [lo, hi) as the decoder's outputs (what wire.phase2b_rows takes)"""
        hi = self.n if hi is None else hi
        return dict(kind=np.full(hi - lo, PHASE2B, np.int32), group_index=self.group_index[lo:hi].copy(),
                    acceptor_index=self.acceptor_index[lo:hi].copy(), slot=self.slot[lo:hi].copy(),
                    round=self.round[lo:hi].copy())


def oracle_run(pyoracle, stream):
    """the stream message at a time through the oracle's ProxyLeader.handlePhase2b: (system, chosen [(index, slot, round,
    value)], states {(slot, round): 1 Pending / 2 Done})"""
    ref = pyoracle.System(pyoracle.make_config(**stream.kw))
    for s, r, v in zip(stream.open_slot.tolist(), stream.open_round.tolist(), stream.open_value.tolist()):
        assert ref.proxy_handle_phase2a(s, r, v)
    chosen = []
    states = {(s, r): 1 for s, r in zip(stream.open_slot.tolist(), stream.open_round.tolist())}
    for i, (b, s, r) in enumerate(zip(stream.bit.tolist(), stream.slot.tolist(), stream.round.tolist())):
        rc, v = ref.proxy_handle_phase2b(b, s, r)
        assert rc in (0, 1, 2)
        if rc == 1:
            chosen.append((i, s, r, v))
            states[(s, r)] = 2
    return ref, chosen, states
