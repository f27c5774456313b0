"""epaxos_cluster.py -- TEST INFRASTRUCTURE ONLY: a seeded cluster of hosted EPaxos replicas under random schedules.

Every replica is one node; the messages on the network are what the nodes themselves emit.  Two node kinds sit behind one
interface (propose / deliver / timer / recover / accept_decided / state / view):

    ModelCluster   one ClusterModel for all n replicas -- tests/epaxos_recovery_model.py's RecoveryModel on the multi-key
                   replicas of tests/epaxos_multikey_sets.py, with lead / lead_accept of tests/epaxos_leader_mk_model.py and the
                   one-message handlers of tests/epaxos_inbox_mk_model.py plus the eager leader-state drops of LeaderModel
    GpuNode        one context per replica r that hosts only r: frames in, frames out (see its docstring for the recipe)

`Simulation` owns the network (one queue per ordered pair, fifo or not, drops, duplicates, silenced replicas, the slow-path
timer and recoveries as injected events, a bounded heal phase), the global command table (the part of each replica's host),
the census of what a run reached and -- when it is given GPU nodes beside the model -- the differential check after every
delivered run.  The end-of-run invariants (`check_invariants`, `check_execution`) read a plain view of the committed instances,
built from GPU read-backs alone or from the model.

A message on the network is (tag, tuple):
    "in"  (kind, to, leader, number, ballot_ordering, ballot_replica, keys, is_set, triple_id, watermarks, values_end)
          the layout of tests/epaxos_inbox_mk_model.py; keys are the GLOBAL key numbers of the command table
    "re"  (kind, to, leader, number, ballot_ordering, ballot_replica, replica_index, seq, watermarks, values_end)
          the layout of tests/epaxos_leader_model.py's replies; kind 3 (the timer) never travels
    "ok"  (to, leader, number, ballot_ordering, ballot_replica, replica_index, status, vote_ordering, vote_replica,
           triple_id, seq, watermarks, values_end)      the layout of tests/epaxos_recovery_model.py's prepare_oks

Nothing here imports the GPU package at module level.
"""
import collections
import os
import random

import numpy as np

from oracle import depgraph as DG
from oracle import epaxos_sets as ES
from tests import epaxos_cmd_cases as CC
from tests import epaxos_inbox_mk_model as IMK
from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_streams as IS
from tests import epaxos_leader_mk_model as LMK
from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as LS
from tests import epaxos_multikey_sets as MK
from tests import epaxos_recovery_model as R
from tests import epaxos_recovery_streams as RS

NK, NI = 4, 64
NOOP_TID = 0
MAX_TRIPLES = 1 << 10
PER_COLUMN = 40                     # instances per leader column
BURST_MAX = 130                     # a delivery is 1 .. BURST_MAX messages: bursts cross 64 and 65
TIMER_DELAY, RECOVERY_DELAY, SILENCE_STEPS = 3, 14, 14
HEAL_ROUNDS = 60                    # the heal phase stops after this many rounds, committed or not
FAULTS = dict(drop=0.03, duplicate=0.04, silence=0.08)

FORM_SWITCHES = ("FPX_EPX_CMDS_WORDS", "FPX_EPX_ENC_DIRECT")     # the store's copy form, the encoder's emit form
OTHER_FORMS = {k: "1" for k in FORM_SWITCHES}                        # word copies, direct emit

KINDS = {16: IM.IN_PRE_ACCEPT, 18: IM.IN_ACCEPT, 20: IM.IN_COMMIT, 21: IM.IN_PREPARE}
WIRE_KIND = {v: k for k, v in KINDS.items()}
WIRE_REPLY = {17: M.PRE_ACCEPT_OK, 19: M.ACCEPT_OK, 23: M.NACK}
WIRE_STATUS = {R.NOT_SEEN: 0, R.PRE_ACCEPTED: 1, R.ACCEPTED: 2}       # PrepareOk.status on the wire
MODEL_STATUS = {v: k for k, v in WIRE_STATUS.items()}


# ---- frames (shared with tests/test_gpu_epaxos_wire_replica_tick.py and the tests that import from it) -----------------------
def command_of(x):
    """the serialised CommandOrNoop of a message: a list without keys travels as a Noop, a get or a set without keys"""
    keys = [b"k%d" % k for k in x[6]]
    if not keys and x[8] % 3 == 0:
        return CC.NOOP
    return (CC.set_ if x[7] else CC.get)(keys, client_id=x[8])


def frame(wire, x, command=None):
    kind, to, L, inst, bo, br, keys, is_set, tid, w, end = x
    if kind == IM.IN_PREPARE:
        return wire.epaxos_encode(21, (L, inst), ballot=(bo, br))
    values = [(L, v) for v in range(inst + 1, end)] if end else []
    cmd = command_of(x) if command is None else command
    kw = dict(command=cmd, sequence_number=tid & 0xff, deps=w, values=values)
    if kind == IM.IN_COMMIT:
        return wire.epaxos_encode(20, (L, inst), **kw)
    return wire.epaxos_encode(WIRE_KIND[kind], (L, inst), ballot=(bo, br), **kw)


# ---- the command table: what every replica's host knows of the commands (engine.triples on the JVM) ---------------------------
class Commands:
    """one global table: every distinct command has one triple id; triple 0 is the Noop"""

    def __init__(self):
        self.keys, self.is_set, self.bytes, self.by_bytes = {}, {}, {}, {}
        self._add((), 0, CC.NOOP)

    def _add(self, keys, is_set, raw):
        tid = len(self.bytes)
        assert tid < MAX_TRIPLES and raw not in self.by_bytes
        self.keys[tid], self.is_set[tid], self.bytes[tid], self.by_bytes[raw] = tuple(keys), int(is_set), raw, tid
        return tid

    def new(self, keys, is_set):
        tid = len(self.bytes)
        raw = (CC.set_ if is_set else CC.get)([b"k%d" % k for k in keys], client_id=tid)
        return self._add(keys, is_set, raw)

    def multi(self, tid):
        return len(set(self.keys[tid])) > 1

    def conflict(self, a, b):
        return bool(set(self.keys[a]) & set(self.keys[b])) and bool(self.is_set[a] or self.is_set[b])

    def arrays(self):
        """the table as the plain arrays of wire.epx_encode_replica_replies_cmds"""
        off, ln, arena = np.full(MAX_TRIPLES, -1, np.int64), np.zeros(MAX_TRIPLES, np.int32), bytearray()
        for t, c in self.bytes.items():
            off[t], ln[t] = len(arena), len(c)
            arena += c
        return off, ln, np.frombuffer(bytes(arena), np.uint8)


def msg_in(cmds, kind, to, inst, ballot, tid, we):
    w, end = we
    if kind == IM.IN_PREPARE:
        return ("in", (kind, to, inst[0], inst[1], ballot[0], ballot[1], (), 0, -1, [0] * len(w), 0))
    if kind == IM.IN_COMMIT:
        ballot = (-1, -1)
    return ("in", (kind, to, inst[0], inst[1], ballot[0], ballot[1], cmds.keys[tid], cmds.is_set[tid], tid, list(w), int(end)))


def encode_msg(wire, cmds, msg):
    """a network message as the frame its sender's host builds with wire.epaxos_encode"""
    tag, x = msg
    if tag == "in":
        return frame(wire, x[:8] + (0,) + x[9:], command=None if x[0] == IM.IN_PREPARE else cmds.bytes[x[8]])
    if tag == "re":
        kind, to, L, num, bo, br, q, seq, w, end = x
        if kind == M.PRE_ACCEPT_OK:
            return wire.epaxos_encode(17, (L, num), ballot=(bo, br), replica_index=q, sequence_number=seq, deps=w,
                                      values=[(L, v) for v in range(num + 1, end)] if end else [])
        if kind == M.ACCEPT_OK:
            return wire.epaxos_encode(19, (L, num), ballot=(bo, br), replica_index=q)
        return wire.epaxos_encode(23, (L, num), ballot=(bo, br))
    to, L, num, bo, br, q, status, vo, vr, tid, seq, w, end = x
    if status == R.NOT_SEEN:
        return wire.epaxos_encode(22, (L, num), ballot=(bo, br), replica_index=q, vote_ballot=(vo, vr), status=0)
    return wire.epaxos_encode(22, (L, num), ballot=(bo, br), replica_index=q, vote_ballot=(vo, vr), status=WIRE_STATUS[status],
                              command=cmds.bytes[tid], sequence_number=seq, deps=w,
                              values=[(L, v) for v in range(num + 1, end)] if end else [])


def decode_frames(wire, cmds, n, frames, src, dst):
    """frames that replica `src` sends to `dst`, decoded on the host -> network messages.  A command travels as bytes: its
    triple id is the table's.  (A Nack names no sender on the wire; the tuple carries the sender the transport knows.)"""
    if not frames:
        return []
    dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=n)
    assert dec["status_code"] == 0, (dec["status_code"], dec["bad_index"])
    out = []
    for i in range(len(frames)):
        kind = int(dec["kind"][i])
        L, num = int(dec["instance_leader"][i]), int(dec["instance_number"][i])
        bo, br = int(dec["ballot_ordering"][i]), int(dec["ballot_replica"][i])
        has_deps = int(dec["deps_num_replicas"][i]) >= 0
        w = [int(v) for v in dec["deps_watermark"][i]] if has_deps else [0] * n
        end = int(dec["deps_values_end"][i]) if has_deps else 0
        tid = -1
        if int(dec["cmd_len"][i]) >= 0:
            o = int(dec["cmd_off"][i])
            tid = cmds.by_bytes[dec["buf"][o:o + int(dec["cmd_len"][i])].tobytes()]
        if kind in KINDS:
            if kind == 21:
                out.append(msg_in(cmds, IM.IN_PREPARE, dst, (L, num), (bo, br), -1, ([0] * n, 0)))
            else:
                out.append(msg_in(cmds, KINDS[kind], dst, (L, num), (bo, br), tid, (w, end)))
        elif kind in WIRE_REPLY:
            k = WIRE_REPLY[kind]
            q = src if k == M.NACK else int(dec["replica_index"][i])
            seq = int(dec["sequence_number"][i]) if k == M.PRE_ACCEPT_OK else 0
            out.append(("re", (k, dst, L, num, bo, br, q, seq, w if k == M.PRE_ACCEPT_OK else [0] * n,
                               end if k == M.PRE_ACCEPT_OK else 0)))
        else:
            assert kind == 22, kind
            status = MODEL_STATUS[int(dec["status"][i])]
            vo, vr = int(dec["vote_ballot_ordering"][i]), int(dec["vote_ballot_replica"][i])
            seq = int(dec["sequence_number"][i]) if status != R.NOT_SEEN else 0
            out.append(("ok", (dst, L, num, bo, br, int(dec["replica_index"][i]), status, vo, vr, tid, seq, w, end)))
    return out


def classes_of(burst):
    """a delivery split, in order, into maximal runs of one class"""
    runs = []
    for src, msg in burst:
        if runs and runs[-1][0] == msg[0]:
            runs[-1][1].append((src, msg))
        else:
            runs.append((msg[0], [(src, msg)]))
    return runs


# ---- the model of all n replicas ------------------------------------------------------------------------------------------------
class ClusterModel(R.RecoveryModel):
    """RecoveryModel over multi-key replicas; the one-message replica handlers of InboxMkModel with LeaderModel's eager drops.
    `fast_short`: the deliberately WRONG variant of the negative control -- a fast quorum one replica short"""
    lead = LMK.LeaderMkModel.lead
    lead_accept_mk = LMK.LeaderMkModel.lead_accept
    _valid, refuses = LMK.LeaderMkModel._valid, LMK.LeaderMkModel.refuses
    handle_preaccept, handle_commit = MK.EPaxos.handle_preaccept, MK.EPaxos.handle_commit
    handle_accept, valid = IMK.InboxMkModel.handle_accept, IMK.InboxMkModel.valid
    _deliver = IMK.InboxMkModel.deliver

    def __init__(self, n, fast_short=False):
        super().__init__(n, NK, NI)
        self.replicas = [MK.Replica(r, n, NK) for r in range(n)]
        if fast_short:
            self.fast -= 1

    def _slow_path(self, to, inst, st):
        res = super()._slow_path(to, inst, st)
        self.leader_states[to][inst].keys = st.keys          # (the Accepting state keeps the list, as the mk model's does)
        return res

    def deliver_in(self, msg):
        """one PreAccept / Accept / Commit / Prepare at replica msg[1]: InboxMkModel's row, and the leader state of the instance
        dropped where the reference drops it (:1239-1242, :1480-1483, :1645-1648, commit :831)"""
        assert self.valid(msg), msg
        kind, to, inst, ballot = msg[0], msg[1], (msg[2], msg[3]), (msg[4], msg[5])
        if kind == IM.IN_PREPARE:
            st = self.leader_states[to].get(inst)
            if isinstance(st, R.Preparing) and ballot > st.ballot:
                self.census["prepare_while_preparing"] += 1
            self._yield_to(to, inst, ballot)
        row = self._deliver(msg)
        if row[0] in (IM.RI_PRE_ACCEPT_OK, IM.RI_ACCEPT_OK):
            self._yield_to(to, inst, ballot)
        elif row[0] == IM.RI_LEARNT:
            self.leader_states[to].pop(inst, None)
        return row


def _model_rows_replies(n, msgs, out):
    rows = []
    for msg, (outcome, seq, d, tid) in zip(msgs, out):
        w, end = ([0] * n, 0) if d is None else LS.encode_deps(n, (msg[2], msg[3]), d)
        rows.append((outcome, seq, w, end, tid))
    return rows


class ModelCluster:
    def __init__(self, n, cmds, fast_short=False, as_intended=True):
        self.n, self.cmds, self.as_intended = n, cmds, as_intended
        self.model = ClusterModel(n, fast_short)

    def close(self):
        pass

    # -- a client's commands at replica r: transitionToPreAcceptPhase, the PreAccepts to every peer
    def propose(self, r, items, avoid=0):
        """items: (instance, ballot ordering, triple id) -> (rows, messages as (destination, message))"""
        c = self.cmds
        st, deps = self.model.lead([(i[0], i[1], r, bo, c.keys[t], c.is_set[t], t, avoid) for (i, bo, t) in items])
        assert st == M.OK, st
        rows = [LS.encode_deps(self.n, i, d) for (i, _, _), d in zip(items, deps)]
        return rows, self._to_peers(r, IM.IN_PRE_ACCEPT, items, rows)

    def _to_peers(self, r, kind, items, deps_rows):
        out = []
        for (inst, bo, t), we in zip(items, deps_rows):
            out += [(p, msg_in(self.cmds, kind, p, inst, (bo, r), t, we)) for p in range(self.n) if p != r]
        return out

    def recover(self, r, insts):
        st, out = self.model.recover([(i[0], i[1], r) for i in insts])
        assert st == M.OK, st
        msgs = []
        for inst, row in zip(insts, out):
            if row[0] == R.RV_PREPARING:
                msgs += [(p, msg_in(self.cmds, IM.IN_PREPARE, p, inst, (row[1], r), -1, ([0] * self.n, 0)))
                         for p in range(self.n) if p != r]
        return [tuple(x) for x in out], msgs

    def accept_decided(self, r, items):
        """transitionToAcceptPhase with the triples a recovery chose: items (instance, ballot ordering, triple id, seq, (w, end))"""
        c = self.cmds
        st = self.model.lead_accept_mk([(i[0], i[1], r, bo, c.keys[t], c.is_set[t], t, seq, M.deps_from_message(self.n, i, w, end))
                                        for (i, bo, t, seq, (w, end)) in items])
        assert st == M.OK, st
        return [st], self._to_peers(r, IM.IN_ACCEPT, [x[:3] for x in items], [x[4] for x in items])

    def timer(self, r, inst, bo):
        return self.deliver(r, "re", [(r, ("re", (M.SLOW_PATH_TIMER, r, inst[0], inst[1], bo, r, r, 0, [0] * self.n, 0)))])

    def timer_ok(self, r, inst):
        st = self.model.leader_states[r].get(inst)
        return isinstance(st, M.PreAccepting) and len(st.responses) >= self.model.slow

    def deliver(self, r, tag, run):
        """one run of one class at replica r, message at a time -> (rows, messages)"""
        n, model, msgs = self.n, self.model, [m[1] for _, m in run]
        assert all((x[0] if tag == "ok" else x[1]) == r for x in msgs)
        out = []
        if tag == "in":
            rows = []
            for (src, _), x in zip(run, msgs):
                row = tuple(model.deliver_in(x))
                rows.append(row)
                out += self._reply(r, src, x, row)
            return rows, out
        if tag == "re":
            st, res, decided = model.replies(msgs)
            assert st == M.OK, (st, msgs)
            rows = _model_rows_replies(n, msgs, res)
            return (rows, decided), out + self._decisions(r, msgs, rows, decided)
        st, res, decided = model.prepare_oks(msgs, self.as_intended)
        assert st == M.OK, (st, msgs)
        rows = []
        for x, (outcome, src, tid, ballot, seq, d) in zip(msgs, res):
            w, end = RS.enc_deps(n, (x[1], x[2]), d) if outcome == R.RC_ACCEPT else ([0] * n, 0)
            rows.append((outcome, src, tid, ballot, seq, w, end))
        return (rows, decided), out

    def _reply(self, r, src, x, row):
        n, inst, ballot = self.n, (x[2], x[3]), (x[4], x[5])
        outcome, ob, status, deps, tid = row
        if outcome in (IM.RI_PRE_ACCEPT_OK, IM.RI_PRE_ACCEPT_OK_AGAIN):
            w, end = LS.encode_deps(n, inst, deps)
            return [(src, ("re", (M.PRE_ACCEPT_OK, src, inst[0], inst[1], ballot[0], ballot[1], r, 0, w, end)))]
        if outcome in (IM.RI_ACCEPT_OK, IM.RI_ACCEPT_OK_AGAIN):
            return [(src, ("re", (M.ACCEPT_OK, src, inst[0], inst[1], ballot[0], ballot[1], r, 0, [0] * n, 0)))]
        if outcome == IM.RI_NACK:
            return [(src, ("re", (M.NACK, src, inst[0], inst[1], ob >> 3, ob & 7, r, 0, [0] * n, 0)))]
        if outcome == IM.RI_COMMIT_BACK:
            return [(src, msg_in(self.cmds, IM.IN_COMMIT, src, inst, (-1, -1), tid, LS.encode_deps(n, inst, deps)))]
        if outcome == IM.RI_PREPARE_OK:
            if status == 0:
                return [(src, ("ok", (src, inst[0], inst[1], ballot[0], ballot[1], r, 0, -1, -1, -1, 0, [0] * n, 0)))]
            w, end = LS.encode_deps(n, inst, deps)
            return [(src, ("ok", (src, inst[0], inst[1], ballot[0], ballot[1], r, status, ob >> 3, ob & 7, tid, 0, w, end)))]
        return []

    def _decisions(self, r, msgs, rows, decided):
        """an ACCEPT outcome -> Accept to every peer, a commit -> Commit to every peer"""
        out = []
        for i in decided:
            outcome, seq, w, end, tid = rows[i]
            inst, ballot = (msgs[i][2], msgs[i][3]), (msgs[i][4], msgs[i][5])
            kind = IM.IN_ACCEPT if outcome == M.ACCEPT else IM.IN_COMMIT
            out += [(p, msg_in(self.cmds, kind, p, inst, ballot, tid, (w, end))) for p in range(self.n) if p != r]
        return out

    # -- read-backs
    def state(self, r, insts):
        return model_state(self.model, r, insts)

    def view(self, r, insts):
        """the committed instances of replica r: instance -> (triple id, (watermarks, values_end))"""
        out = {}
        for inst in insts:
            e = self.model.replicas[r].cmd_log.get(inst)
            if e is not None and e.kind == ES.COMMITTED:
                out[inst] = (e.triple_id, LS.encode_deps(self.n, inst, e.deps))
        return out


def model_state(model, r, insts):
    """replica r as the GPU read-backs show it (tests/epaxos_recovery_streams.model_state, with the key word of a key list)"""
    n, out = model.n, {}
    for inst in insts:
        e = model.replicas[r].cmd_log.get(inst)
        if e is None:
            entry, deps = (0, -1, -1, -1), None
        else:
            entry = (e.kind, R.enc(e.ballot), R.enc(e.vote_ballot), e.triple_id)
            deps = None if e.deps is None else LS.encode_deps(n, inst, e.deps)
        st = model.leader_states[r].get(inst)
        if st is None:
            ls = (0,)
        elif isinstance(st, M.PreAccepting):
            resp = {q: (s,) + tuple(LS._flat(LS.encode_deps(n, inst, d))) for q, (s, d) in st.responses.items()}
            ls = (1, R.enc(st.ballot), int(st.avoid_fast_path), st.triple_id, st.keys, int(st.is_set), resp)
        elif isinstance(st, M.Accepting):
            s, d = st.triple
            ls = (2, R.enc(st.ballot), st.triple_id, st.keys, int(st.is_set), sorted(st.responses),
                  (s,) + tuple(LS._flat(LS.encode_deps(n, inst, d))))
        else:
            ls = (3, R.enc(st.ballot), {q: (p.status, R.enc(p.vote_ballot), p.triple_id, p.seq) +
                                        tuple(LS._flat(LS.encode_deps(n, inst, p.deps))) for q, p in st.responses.items()})
        out[inst] = (entry, deps, ls)
    rep = model.replicas[r]
    index = {k: (list(rep.gets[k]), list(rep.sets[k])) for k in range(NK)}
    return out, R.enc(rep.largest_ballot), index


# ---- one GPU context per replica ----------------------------------------------------------------------------------------------
class GpuNode:
    """replica r hosted alone on one context (`to` / `at` = r in every call), the loop of a hosted replica:

        PreAccept, Accept, Commit, Prepare frames -> wire_replica_tick_bytes; the reply frames it returns go back to the senders,
            the replies it marks deferred (reply_kind 2) are built on the host by wire.epx_encode_replica_replies_cmds from the
            tick's own struct-of-arrays outputs and the host's command table
        PreAcceptOk, AcceptOk, Nack frames        -> wire_leader_tick; an ACCEPT outcome -> Accept frames, a commit -> Commit frames
        PrepareOk frames                          -> decoded on the host, recovery_replies; its decisions -> lead_mk(avoid_fast_path)
                                                     / lead_accept_mk
        a client's command                        -> keys_intern, lead_mk -> PreAccept frames;  recover -> Prepare frames

    The host-pointer form of every call.  `raw` keeps, per destination, the frames this node emitted, so that what a peer parses
    are the bytes this context produced."""

    def __init__(self, wire, n, r, cmds, env=None):
        from frankenpaxos_amd.epaxos import EPaxos

        forms = dict.fromkeys(FORM_SWITCHES)        # fpx_epx_create reads them: set around it only
        forms.update(env or {})
        saved = {k: os.environ.pop(k, None) for k in forms}
        os.environ.update({k: v for k, v in forms.items() if v is not None})
        try:
            self.epx = EPaxos(n, NK, num_instances=NI, leader_state=True, recovery=True)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.epx.keys_enable(1 << 12)
        self.epx.cmds_enable(MAX_TRIPLES, 1 << 18)
        self.wire, self.n, self.r, self.cmds = wire, n, r, cmds
        self.key_ids, self.carried = {}, set()      # the host's own books: key string -> id in first-occurrence order; triples of frames
        self.deferred = 0
        self.sent = []                              # every frame emitted, in order: (destination, bytes)

    def close(self):
        self.epx.close()

    def _see_keys(self, tid):
        for k in self.cmds.keys[tid]:
            self.key_ids.setdefault(b"k%d" % k, len(self.key_ids))

    def _lists(self, tids):
        """the key ids of the commands, from the device's table (a hosted replica interns before it leads)"""
        flat = [b"k%d" % k for t in tids for k in self.cmds.keys[t]]
        for t in tids:
            self._see_keys(t)
        if not flat:
            return [[] for _ in tids]
        st, ids = self.epx.keys_intern(flat)
        assert st == 0 and [int(v) for v in ids] == [self.key_ids[k] for k in flat], (st, ids)
        out, at = [], 0
        for t in tids:
            k = len(self.cmds.keys[t])
            out.append([int(v) for v in ids[at:at + k]])
            at += k
        return out

    def _emit(self, msgs):
        """(destination, message) -> frames, remembered; the messages go on as they are"""
        for dst, msg in msgs:
            self.sent.append((dst, encode_msg(self.wire, self.cmds, msg)))
        return msgs

    def _to_peers(self, kind, items, deps_rows):
        out = []
        for (inst, bo, t), we in zip(items, deps_rows):
            out += [(p, msg_in(self.cmds, kind, p, inst, (bo, self.r), t, we)) for p in range(self.n) if p != self.r]
        return self._emit(out)

    def propose(self, r, items, avoid=0):
        c, m = self.cmds, len(items)
        tids = [t for (_, _, t) in items]
        st, deps, dend = self.epx.lead_mk([i[0] for (i, _, _) in items], [i[1] for (i, _, _) in items], [r] * m,
                                          [bo for (_, bo, _) in items], self._lists(tids), [c.is_set[t] for t in tids], tids,
                                          [avoid] * m)
        assert st == 0, st
        rows = [([int(v) for v in deps[i]], int(dend[i])) for i in range(m)]
        return rows, self._to_peers(IM.IN_PRE_ACCEPT, items, rows)

    def recover(self, r, insts):
        st, outcome, ord_, os_, ov, ot = self.epx.recover([i[0] for i in insts], [i[1] for i in insts], [r] * len(insts))
        assert st == 0, st
        rows = [(int(outcome[i]), int(ord_[i]), int(os_[i]), int(ov[i]), int(ot[i])) for i in range(len(insts))]
        msgs = []
        for inst, row in zip(insts, rows):
            if row[0] == R.RV_PREPARING:
                msgs += [(p, msg_in(self.cmds, IM.IN_PREPARE, p, inst, (row[1], r), -1, ([0] * self.n, 0)))
                         for p in range(self.n) if p != r]
        return rows, self._emit(msgs)

    def accept_decided(self, r, items):
        c, m = self.cmds, len(items)
        tids = [x[2] for x in items]
        st = self.epx.lead_accept_mk([x[0][0] for x in items], [x[0][1] for x in items], [r] * m, [x[1] for x in items],
                                     self._lists(tids), [c.is_set[t] for t in tids], tids, [x[3] for x in items],
                                     np.asarray([x[4][0] for x in items], np.int32), [x[4][1] for x in items])
        assert st == 0, st
        return [st], self._to_peers(IM.IN_ACCEPT, [x[:3] for x in items], [x[4] for x in items])

    def timer(self, r, inst, bo):
        msgs = [(M.SLOW_PATH_TIMER, r, inst[0], inst[1], bo, r, r, 0, [0] * self.n, 0)]
        res = self.epx.leader_replies(*LS.burst_arrays(self.n, msgs))
        return self._leader_rows(msgs, res)

    def _leader_rows(self, msgs, res):
        st, outcome, oseq, odeps, oend, otr, dec = res[:7]
        assert st == 0, (st, res[7:])
        rows = [(int(outcome[i]), int(oseq[i]), [int(v) for v in odeps[i]], int(oend[i]), int(otr[i])) for i in range(len(msgs))]
        decided = [int(v) for v in dec]
        out = []
        for i in decided:
            o, seq, w, end, tid = rows[i]
            inst, ballot = (msgs[i][2], msgs[i][3]), (msgs[i][4], msgs[i][5])
            kind = IM.IN_ACCEPT if o == M.ACCEPT else IM.IN_COMMIT
            out += [(p, msg_in(self.cmds, kind, p, inst, ballot, tid, (w, end))) for p in range(self.n) if p != self.r]
        return (rows, decided), self._emit(out)

    def deliver(self, r, tag, run, frames):
        """frames: the bytes of the run's messages, as their senders emitted them"""
        n, wire, msgs = self.n, self.wire, [m[1] for _, m in run]
        m = len(msgs)
        if tag == "re":
            return self._leader_rows(msgs, self.epx.wire_leader_tick(frames, [r] * m))
        if tag == "ok":
            dec = decode_frames(wire, self.cmds, n, frames, -1, r)
            assert [x[1] for x in dec] == msgs                   # (the host decoder on the sender's bytes gives the message back)
            res = self.epx.recovery_replies(*RS.prepare_ok_arrays(n, msgs), as_intended=True)
            st, rows, decided = RS.gpu_rows(n, res)
            assert st == 0, st
            return (rows, decided), []
        triple = [x[8] for x in msgs]
        for x in msgs:
            if x[0] != IM.IN_PREPARE:
                self._see_keys(x[8])
                self.carried.add(x[8])
        got = self.epx.wire_replica_tick_bytes(frames, [r] * m, max_pairs=8 * m + 8, triple_id=triple, out_cap=m * 640)
        assert got["status_code"] == 0, (got["status_code"], got["bad_index"], got["totals"])
        soa = [got[k] for k in ("outcome", "out_ballot", "out_status", "out_deps", "out_values_end", "out_triple")]
        renamed = [x[:6] + (0,) + x[7:] for x in msgs]
        rows = [tuple(x) for x in IS.decode_outputs(n, renamed, soa)]
        replies = list(got["replies"])
        late = [i for i in range(m) if got["reply_kind"][i] == 2]
        if late:                                                 # the host's part, from the tick's own outputs
            dec = wire.epaxos_decode_replica_inbound_folded(frames, num_replicas=n)
            host = wire.epx_encode_replica_replies_cmds(
                n, soa[5], self.cmds.arrays(), to=[r] * m, leader=dec["instance_leader"], number=dec["instance_number"],
                ballot_ordering=dec["ballot_ordering"], ballot_replica=dec["ballot_replica"], outcome=soa[0], out_ballot=soa[1],
                out_status=soa[2], out_deps=soa[3], out_values_end=soa[4])
            assert host["status_code"] == 0 and all(host["reply_kind"][i] == 1 for i in late), host["reply_kind"]
            for i in late:
                replies[i] = host["replies"][i]
            self.deferred += len(late)
        out = []
        for i, (src, _) in enumerate(run):
            assert (len(replies[i]) > 0) == (got["reply_kind"][i] != 0)
            if replies[i]:
                self.sent.append((src, replies[i]))
                out += [(src, x) for x in decode_frames(wire, self.cmds, n, [replies[i]], r, src)]
        return rows, out

    # -- read-backs
    def state(self, r, insts):
        epx, n = self.epx, self.n
        names = epx.keys_read()
        assert names == sorted(self.key_ids, key=self.key_ids.get), (names, self.key_ids)
        glob = {i: int(k[1:]) for i, k in enumerate(names)}
        out = {}
        for inst in insts:
            kind, ballot, vote, tid, _ = epx.read_cmdlog(r, inst[0], inst[1])
            d, dend = epx.read_cmdlog_deps(r, inst[0], inst[1])
            deps = None if (kind in (0, 1) or d[0] == -1) else ([int(v) for v in d], dend)
            if kind == 0:
                ballot = vote = tid = -1
            head, resp = epx.read_leader_state(r, inst[0], inst[1])
            phase, lb, avoid, ltid, key, is_set, mask = head[:7]
            # the key word of the leader state, held against the command's list: -1, the one key, or KEY_LIST
            if phase in (1, 2):
                keys = self.cmds.keys[ltid]
                assert key == LMK.key_word([self.key_ids[b"k%d" % k] for k in keys]), (inst, key, keys)
            if phase == 0:
                ls = (0,)
            elif phase == 1:
                ls = (1, lb, avoid, ltid, keys, is_set, {q: tuple(int(v) for v in resp[q]) for q in range(n) if (mask >> q) & 1})
            elif phase == 2:
                ls = (2, lb, ltid, keys, is_set, [q for q in range(n) if (mask >> q) & 1], tuple(int(v) for v in resp[r]))
            else:
                rs = epx.read_recovery_state(r, inst[0], inst[1])
                assert all((rs[q, 0] >= 0) == bool((mask >> q) & 1) for q in range(n))
                ls = (3, lb, {q: tuple(int(v) for v in rs[q]) + tuple(int(v) for v in resp[q]) for q in range(n) if (mask >> q) & 1})
            out[inst] = ((kind, ballot, vote, tid), deps, ls)
        index = {k: ([0] * n, [0] * n) for k in range(NK)}
        for i in range(len(names)):
            g, s = epx.read_index(r, i)
            index[glob[i]] = ([int(v) for v in g], [int(v) for v in s])
        return out, epx.read_cmdlog(r, 0, 0)[4], index

    def view(self, r, insts):
        out = {}
        for inst in insts:
            kind, _, _, tid, _ = self.epx.read_cmdlog(r, inst[0], inst[1])
            if kind == ES.COMMITTED:
                d, dend = self.epx.read_cmdlog_deps(r, inst[0], inst[1])
                out[inst] = (tid, ([int(v) for v in d], int(dend)))
        return out

    def check_store(self):
        """the command store and the key table against the host's own books"""
        assert self.epx.cmds_stats()[2:] == (0, 0), self.epx.cmds_stats()
        for t in sorted(self.carried):
            assert self.epx.cmds_read(t) == self.cmds.bytes[t], (self.r, t)
        assert self.epx.cmds_stats()[0] == len(self.carried)
        assert self.epx.keys_read() == sorted(self.key_ids, key=self.key_ids.get)


class GpuCluster:
    """n GpuNodes behind ModelCluster's interface; the frames of a delivered run are the senders' own bytes"""

    def __init__(self, wire, n, cmds, env=None):
        self.n, self.cmds, self.wire = n, cmds, wire
        self.nodes = [GpuNode(wire, n, r, cmds, env) for r in range(n)]
        self.raw = collections.defaultdict(collections.deque)     # (source, destination, message) -> the frames emitted for it
        self.marks = [0] * n

    def close(self):
        for node in self.nodes:
            node.close()

    def _collect(self, r, msgs):
        """file the frames node r emitted since the last call under the messages they carry"""
        node = self.nodes[r]
        new = node.sent[self.marks[r]:]
        self.marks[r] = len(node.sent)
        assert len(new) == len(msgs), (len(new), len(msgs))
        for (dst, raw), (dst2, msg) in zip(new, msgs):
            assert dst == dst2
            self.raw[(r, dst, _key(msg))].append(raw)
        return msgs

    def propose(self, r, items, avoid=0):
        rows, out = self.nodes[r].propose(r, items, avoid)
        return rows, self._collect(r, out)

    def recover(self, r, insts):
        rows, out = self.nodes[r].recover(r, insts)
        return rows, self._collect(r, out)

    def accept_decided(self, r, items):
        rows, out = self.nodes[r].accept_decided(r, items)
        return rows, self._collect(r, out)

    def timer(self, r, inst, bo):
        rows, out = self.nodes[r].timer(r, inst, bo)
        return rows, self._collect(r, out)

    def deliver(self, r, tag, run):
        frames = []
        for src, msg in run:
            q = self.raw.get((src, r, _key(msg)))                # (a duplicate on the network is the same bytes again;
            frames.append(q[0] if q else encode_msg(self.wire, self.cmds, msg))   # a re-broadcast Commit is the host's frame)
        rows, out = self.nodes[r].deliver(r, tag, run, frames)
        return rows, self._collect(r, out)

    def state(self, r, insts):
        return self.nodes[r].state(r, insts)

    def view(self, r, insts):
        return self.nodes[r].view(r, insts)


def _key(msg):
    tag, x = msg
    return (tag,) + tuple(tuple(v) if isinstance(v, list) else v for v in x)


# ---- the simulation -------------------------------------------------------------------------------------------------------------
CENSUS_KEYS = ("fast_commit", "slow_disagreement", "slow_timer", "slow_commit", "nack_at_leader", "back_to_pre_accept",
               "back_to_accept", "back_to_prepare", "ok_status_0", "ok_status_2", "ok_status_3", "decide_noop", "decide_pre_accept",
               "decide_accept_accepted", "decide_accept_popular", "recovery_races_leader", "reply_after_decision",
               "commit_and_prepare_one_burst", "deferred_reply", "mk_fast", "mk_slow", "mk_recovered", "mk_reply",
               "burst_over_64_replica", "burst_over_64_leader", "exec_cycle")


class Mismatch(AssertionError):
    pass


class Simulation:
    """one seeded run.  `primary` is the cluster whose outputs drive the network and the census; `shadow`, if given, gets the
    same calls and must answer the same, run by run (the differential check)"""

    def __init__(self, n, seed, fifo, primary, shadow=None, cmds=None, per_column=PER_COLUMN, faults=FAULTS):
        self.n, self.seed, self.fifo, self.primary, self.shadow = n, seed, fifo, primary, shadow
        self.rng = random.Random(seed * 1000 + n * 10 + int(fifo))
        self.cmds = cmds
        self.per_column, self.faults = per_column, dict(faults)
        self.queues = {(a, b): collections.deque() for a in range(n) for b in range(n) if a != b}
        self.now, self.step_no = 0, 0
        self.next_number = [0] * n
        self.silenced = {}                          # replica -> the step it rejoins at
        self.proposed = collections.defaultdict(set)    # instance -> the triples a client proposed for it
        self.led_at = {}                            # instance -> step it was first led at
        self.open = {}                              # (replica, instance) -> (ballot ordering, avoid): led here, not yet committed here
        self.known = [set() for _ in range(n)]      # instances each replica knows committed (its own decisions, Commits delivered)
        self.commits = {}                           # instance -> (triple id, (w, end)) of the first commit decision: re-broadcast in heal
        self.timers, self.recoveries = [], []       # (due, replica, instance)
        self.oks = collections.defaultdict(dict)    # (replica, instance) -> {responder: status} of the recovery in progress
        self.carried = [set() for _ in range(n)]    # the triples whose bytes a frame brought to each replica
        self.census = collections.Counter()
        self.trace = []
        self.healing = False

    # -- both clusters, compared
    def _both(self, what, r, *args):
        got = getattr(self.primary, what)(r, *args)
        if self.shadow is not None:
            want = getattr(self.shadow, what)(r, *args)
            if _plain(got) != _plain(want):
                raise Mismatch("n=%d seed=%d fifo=%s step %d: %s at replica %d differs\n  args %r\n  got  %r\n  want %r" % (
                    self.n, self.seed, self.fifo, self.step_no, what, r, args, got, want))
        self.trace.append((self.step_no, what, r, _plain(args), _plain(got)))
        return got

    def _send(self, src, msgs):
        for dst, msg in msgs:
            self.queues[(src, dst)].append(msg)

    # -- events
    def propose(self, r, count):
        items = []
        for _ in range(count):
            if self.next_number[r] >= self.per_column:
                break
            inst = (r, self.next_number[r])
            self.next_number[r] += 1
            tid = self._new_command()
            self.proposed[inst].add(tid)
            self.led_at[inst] = self.now
            self.open[(r, inst)] = (0, 0)
            items.append((inst, 0, tid))
        if items:
            rows, out = self._both("propose", r, items, 0)
            self._send(r, out)
            for inst, _, _ in items:
                self.recoveries.append((self.now + RECOVERY_DELAY + self.rng.randrange(RECOVERY_DELAY), inst))

    def _new_command(self):
        rng, p = self.rng, self.rng.random()
        if p < 0.05:
            return NOOP_TID
        if p < 0.10:
            return self.cmds.new((), rng.randrange(2))
        if p < 0.30:
            return self.cmds.new(tuple(rng.randrange(NK) for _ in range(rng.randrange(2, 4))), rng.randrange(2))
        return self.cmds.new((rng.randrange(NK),), int(rng.random() < 0.6))

    def _decided(self, r, msgs, rows, decided, timer=False):
        """bookkeeping and census of one leader run's decisions"""
        for i, (x, row) in enumerate(zip(msgs, rows)):
            inst, o = (x[2], x[3]), row[0]
            if x[0] == M.NACK:
                self.census["nack_at_leader"] += 1
                if o == M.NACK_RECOVER and not any(rc[1:] == (r, inst) for rc in self.recoveries if len(rc) == 3):
                    self.recoveries.append((self.now + 1 + self.rng.randrange(4), r, inst))
            if o == M.IGNORED and x[0] in (M.PRE_ACCEPT_OK, M.ACCEPT_OK) and (inst in self.known[r] or (r, inst, "acc") in self.open):
                self.census["reply_after_decision"] += 1
            if o == M.START_SLOW_PATH_TIMER:
                self.timers.append((self.now + TIMER_DELAY, r, inst, x[4]))
        for i in decided:
            x, (o, seq, w, end, tid) = msgs[i], rows[i]
            inst = (x[2], x[3])
            avoid = self.open.get((r, inst), (0, 0))[1]
            if o == M.FAST_COMMIT:
                self.census["fast_commit"] += 1
                self.census["mk_fast"] += self.cmds.multi(tid)
            elif o == M.ACCEPT:
                self.census["slow_timer" if timer else "slow_disagreement" if not avoid else "slow_avoid"] += 1
                self.census["mk_slow"] += self.cmds.multi(tid)
                self.open[(r, inst, "acc")] = True
            else:
                self.census["slow_commit"] += 1
            if o in (M.FAST_COMMIT, M.SLOW_COMMIT):
                self.known[r].add(inst)
                self.open.pop((r, inst), None)
                self.commits.setdefault(inst, (r, tid, (list(w), end)))

    def fire_timer(self, r, inst, bo):
        if r in self.silenced or not self._model().timer_ok(r, inst):
            return
        (rows, decided), out = self._both("timer", r, inst, bo)
        self._send(r, out)
        self._decided(r, [(M.SLOW_PATH_TIMER, r, inst[0], inst[1], bo, r, r, 0, None, 0)], rows, decided, timer=True)

    def _model(self):
        return self.shadow if self.shadow is not None else self.primary

    def recover(self, r, insts):
        insts = [i for i in insts if i not in self.known[r]]
        if not insts:
            return
        for inst in insts:
            if inst[0] != r and (inst[0], inst) in self.open and inst[0] not in self.silenced:
                self.census["recovery_races_leader"] += 1
        rows, out = self._both("recover", r, insts)
        self._send(r, out)
        for inst, row in zip(insts, rows):
            if row[0] == R.RV_PREPARING:
                self.oks[(r, inst)] = {r: row[2]}
                self.open[(r, inst)] = (row[1], 1)
            elif row[0] == R.RV_COMMITTED:
                self.known[r].add(inst)

    def deliver(self, r, burst):
        for tag, run in classes_of(burst):
            msgs = [m[1] for _, m in run]
            if len(run) > 64:
                self.census["burst_over_64_replica" if tag == "in" else "burst_over_64_leader"] += 1
            if tag == "in":
                rows, out = self._both("deliver", r, tag, run)
                self._replica_census(r, run, rows)
                for dst, msg in out:
                    self.queues[(r, dst)].append(msg)
            elif tag == "re":
                (rows, decided), out = self._both("deliver", r, tag, run)
                self._send(r, out)
                self._decided(r, msgs, rows, decided)
            else:
                (rows, decided), _ = self._both("deliver", r, tag, run)
                self._recovery_decisions(r, msgs, rows, decided)

    def _replica_census(self, r, run, rows):
        learnt = set()
        # (a tick stores the commands of the whole burst before it encodes: a later frame's bytes answer an earlier Prepare)
        self.carried[r].update(x[8] for _, (_, x) in run if x[0] != IM.IN_PREPARE)
        for (src, (_, x)), row in zip(run, rows):
            kind, inst, o = x[0], (x[2], x[3]), row[0]
            if kind == IM.IN_COMMIT:
                learnt.add(inst)
                self.known[r].add(inst)
                self.open.pop((r, inst), None)
            if o == IM.RI_COMMIT_BACK:
                self.census[("back_to_pre_accept", "back_to_accept", None, "back_to_prepare")[kind]] += 1
                if kind == IM.IN_PREPARE and inst in learnt:
                    self.census["commit_and_prepare_one_burst"] += 1
            if o == IM.RI_PREPARE_OK:
                self.census["ok_status_%d" % row[2]] += 1
            if o == IM.RI_COMMIT_BACK or (o == IM.RI_PREPARE_OK and row[2] in (2, 3)):
                self.census["mk_reply"] += self.cmds.multi(row[4])
                # the store holds the bytes only of triples a frame carried here: the rest is the host's to build
                self.census["deferred_reply"] += row[4] not in self.carried[r]

    def _recovery_decisions(self, r, msgs, rows, decided):
        for x in msgs:
            self.oks[(x[0], (x[1], x[2]))][x[5]] = x[6]
        leads, accepts = [], []
        for i in decided:
            x, (outcome, src, tid, ballot, seq, w, end) = msgs[i], rows[i]
            inst = (x[1], x[2])
            if outcome == R.RC_ACCEPT:
                how = "accepted" if self.oks[(r, inst)].get(src) == R.ACCEPTED else "popular"
                self.census["decide_accept_" + how] += 1
                accepts.append((inst, ballot >> 3, tid, seq, (list(w), end)))
                self.open[(r, inst, "acc")] = True
            else:
                self.census["decide_noop" if outcome == R.RC_PRE_ACCEPT_NOOP else "decide_pre_accept"] += 1
                tid = NOOP_TID if outcome == R.RC_PRE_ACCEPT_NOOP else tid
                leads.append((inst, ballot >> 3, tid))
            self.census["mk_recovered"] += self.cmds.multi(tid)
        if leads:
            _, out = self._both("propose", r, leads, 1)
            self._send(r, out)
        if accepts:
            _, out = self._both("accept_decided", r, accepts)
            self._send(r, out)

    # -- the schedule
    def _take(self, r):
        """a burst of 1 .. BURST_MAX pending messages for replica r, with the network's faults"""
        rng = self.rng
        srcs = [s for s in range(self.n) if s != r and s not in self.silenced and self.queues[(s, r)]]
        if not srcs:
            return []
        want, burst = rng.randrange(1, BURST_MAX + 1), []
        if self.fifo:
            while len(burst) < want and srcs:
                s = rng.choice(srcs)
                q = self.queues[(s, r)]
                for _ in range(min(len(q), rng.randrange(1, 2 * BURST_MAX), want - len(burst))):
                    burst.append((s, q.popleft()))
                if not q:
                    srcs.remove(s)
        else:
            pool = [(s, i) for s in srcs for i in range(len(self.queues[(s, r)]))]
            picked = rng.sample(pool, min(want, len(pool)))
            if rng.random() < 0.5:                  # half of the time class by class, so that long runs of one class occur
                picked.sort(key=lambda p: self.queues[(p[0], r)][p[1]][0])
            burst = [(s, self.queues[(s, r)][i]) for s, i in picked]
            gone = set(picked)
            for s in srcs:
                q = self.queues[(s, r)]
                self.queues[(s, r)] = collections.deque(m for i, m in enumerate(q) if (s, i) not in gone)
        if self.healing:
            return burst
        out = []
        for s, m in burst:
            p = rng.random()
            if p < self.faults["drop"]:
                continue
            out.append((s, m))
            if p > 1 - self.faults["duplicate"]:
                out.append((s, m)) if rng.random() < 0.5 else self.queues[(s, r)].append(m)
        return out

    def step(self):
        rng, n = self.rng, self.n
        self.step_no += 1
        self.now += 1
        for r in [r for r, until in self.silenced.items() if until <= self.now]:
            del self.silenced[r]
        if not self.healing and rng.random() < self.faults["silence"] and not self.silenced:
            self.silenced[rng.randrange(n)] = self.now + SILENCE_STEPS + rng.randrange(SILENCE_STEPS)
        awake = [r for r in range(n) if r not in self.silenced]
        if not self.healing:
            for r in awake:
                if self.next_number[r] < self.per_column and rng.random() < 0.35:
                    self.propose(r, rng.choice((1, 1, 2, 3, 5, 36)))
        due = [t for t in self.timers if t[0] <= self.now]
        self.timers = [t for t in self.timers if t[0] > self.now]
        for _, r, inst, bo in due:
            self.fire_timer(r, inst, bo)
        self._fire_recoveries(awake)
        for r in rng.sample(awake, len(awake)):
            if rng.random() < 0.7 or self.healing:
                burst = self._take(r)
                if burst:
                    self.deliver(r, burst)

    def _fire_recoveries(self, awake):
        rng = self.rng
        due = [t for t in self.recoveries if t[0] <= self.now]
        self.recoveries = [t for t in self.recoveries if t[0] > self.now]
        per = collections.defaultdict(list)
        for t in due:
            inst = t[-1]
            if len(t) == 3:                         # a Nack told this replica to recover
                r = t[1]
                if r not in awake:
                    self.recoveries.append((self.now + 2, r, inst))
                    continue
            else:                                   # the instance is old: whoever does not know it committed may recover it
                if all(inst in self.known[q] for q in range(self.n)):
                    continue
                cands = [q for q in awake if inst not in self.known[q] and (q != inst[0] or self.healing)]
                again = 8 + rng.randrange(4) if self.healing else RECOVERY_DELAY + rng.randrange(2 * RECOVERY_DELAY)
                self.recoveries.append((self.now + again, inst))
                if not cands:
                    continue
                # (healing: one recoverer per instance, so that recoveries do not duel for ever)
                r = min(cands, key=lambda q: (q - inst[1]) % self.n) if self.healing else rng.choice(cands)
            if inst not in self.known[r] and inst not in per[r]:
                per[r].append(inst)
        for r in sorted(per):
            self.recover(r, per[r])

    def pending(self):
        return sum(len(q) for q in self.queues.values())

    def all_committed(self):
        return all(inst in self.known[q] for inst in self.led_at for q in range(self.n))

    def run(self):
        """the faulty phase until every column is proposed, then the heal phase; -> rounds the heal phase took"""
        guard = 0
        while min(self.next_number) < self.per_column:
            self.step()
            guard += 1
            assert guard < 2000
        self.healing, self.silenced = True, {}
        self.recoveries = [(self.now + 1 + self.rng.randrange(4),) + t[1:] for t in self.recoveries]
        for rounds in range(HEAL_ROUNDS):
            if self.all_committed() and not self.pending():
                return rounds
            for inst, (src, tid, we) in sorted(self.commits.items()):  # every commit is re-broadcast by who decided it
                for q in range(self.n):
                    if inst not in self.known[q] and q != src and rounds % 4 == 0:
                        self.queues[(src, q)].append(msg_in(self.cmds, IM.IN_COMMIT, q, inst, (-1, -1), tid, we))
            self.step()
        return HEAL_ROUNDS


def _plain(v):
    if isinstance(v, (list, tuple)):
        return tuple(_plain(x) for x in v)
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, np.ndarray):
        return tuple(_plain(x) for x in v.tolist())
    return v


# ---- the end of a run: EPaxos' invariants on a view of the committed instances ---------------------------------------------------
def check_invariants(n, cmds, views, proposed, led):
    """views[r]: instance -> (triple id, (watermarks, values_end)) of what replica r holds committed.  -> the violations, as
    strings (agreement, validity, the dependency invariant, completion)"""
    bad = []
    agreed = {}
    for r, view in enumerate(views):
        for inst, val in view.items():
            val = (val[0], (tuple(val[1][0]), val[1][1]))
            if agreed.setdefault(inst, val) != val:
                bad.append("agreement: %r is %r at replica %d and %r elsewhere" % (inst, val, r, agreed[inst]))
    for inst, (tid, _) in agreed.items():
        if tid != NOOP_TID and tid not in proposed.get(inst, ()):
            bad.append("validity: %r committed triple %d, proposed %r" % (inst, tid, sorted(proposed.get(inst, ()))))
    deps = {inst: M.deps_from_message(n, inst, list(w), end) for inst, (_, (w, end)) in agreed.items()}
    insts = sorted(agreed)
    for i, a in enumerate(insts):
        for b in insts[:i]:
            if cmds.conflict(agreed[a][0], agreed[b][0]) and a not in deps[b] and b not in deps[a]:
                bad.append("dependency: %r and %r conflict and neither depends on the other" % (a, b))
    for inst in sorted(led):
        for r, view in enumerate(views):
            if inst not in view:
                bad.append("completion: %r is not committed at replica %d" % (inst, r))
    return bad


def execution_arrays(n, view):
    insts = sorted(view)
    count = [sum(1 for i in insts if i[0] == l) for l in range(n)]
    assert all(sorted(x for (l2, x) in insts if l2 == l) == list(range(count[l])) for l in range(n)), "the columns are not dense"
    leader, number = [i[0] for i in insts], [i[1] for i in insts]
    deps = np.asarray([view[i][1][0] for i in insts], np.int32).reshape(len(insts), n)
    ends = [view[i][1][1] for i in insts]
    return insts, leader, number, deps, ends, [0] * n, count


def oracle_execution(n, view):
    """oracle/depgraph.py's Tarjan graph on the committed instances in canonical (leader, number) order -> the components in
    execution order, each a list of instances"""
    insts, leader, number, deps, ends, _, _ = execution_arrays(n, view)
    g = DG.TarjanDependencyGraph(DG.InstancePrefixSet(n))
    for i, inst in enumerate(insts):
        g.commit(inst, 0, DG.InstancePrefixSet.from_epx(leader[i], number[i], deps[i], ends[i]))
    comps, blockers = DG.with_deep_stack(g.execute_by_component)
    assert not blockers and sum(len(c) for c in comps) == len(insts), (blockers, len(insts))
    return comps


def check_execution(n, cmds, view, order, component):
    """an execution (order[p] = index into the canonical instance list, component[p]) against the oracle: the same components,
    each contiguous and in (leader, number) order, and every dependency outside a component runs before it.  (Where components
    do not depend on each other the reference leaves the order open, include/fpx.h; so the oracle's own order passes this
    check and any other valid order does.)  -> the executed instances in order"""
    insts = sorted(view)
    comps = oracle_execution(n, view)
    ran = [insts[int(p)] for p in order]
    assert sorted(ran) == insts, "not every committed instance ran exactly once"
    mine = collections.OrderedDict()
    for inst, c in zip(ran, component):
        mine.setdefault(int(c), []).append(inst)
    assert list(mine) == list(range(len(mine))), "components are not numbered in order"
    assert sorted(map(tuple, mine.values())) == sorted(tuple(sorted(c)) for c in comps), "the components differ from the oracle's"
    at = {inst: p for p, inst in enumerate(ran)}
    for c in mine.values():
        assert c == sorted(c) and [at[i] for i in c] == list(range(at[c[0]], at[c[0]] + len(c))), c
        for inst in c:
            w, end = view[inst][1]
            for d in M.deps_from_message(n, inst, list(w), end):
                assert d in at and (d in c or at[d] < at[c[0]]), (inst, d)
    return ran


def conflict_order(cmds, view, ran):
    """the relative order of every pair of conflicting commands: what must be the same at every replica"""
    out = {}
    for i, a in enumerate(ran):
        for b in ran[:i]:
            if cmds.conflict(view[a][0], view[b][0]):
                out[(min(a, b), max(a, b))] = (b, a)
    return out


# ---- one case, start to end -----------------------------------------------------------------------------------------------------
def run_model_case(n, seed, fifo, **variant):
    """the model alone -> (simulation, the model cluster, violations of the invariants, census with the execution's cycles)"""
    cmds = Commands()
    mc = ModelCluster(n, cmds, **variant)
    sim = Simulation(n, seed, fifo, mc, cmds=cmds)
    sim.heal_rounds = sim.run()
    led = sorted(sim.led_at)
    views = [mc.view(r, led) for r in range(n)]
    bad = check_invariants(n, cmds, views, sim.proposed, led)
    census = {k: int(sim.census[k]) for k in CENSUS_KEYS}
    if not bad:                                     # (the execution needs dense, agreed columns)
        comps = oracle_execution(n, views[0])
        order = [i for c in comps for i in c]
        at = {inst: p for p, inst in enumerate(sorted(views[0]))}
        ran = check_execution(n, cmds, views[0], [at[i] for i in order], [k for k, c in enumerate(comps) for _ in c])
        assert ran == order
        census["exec_cycle"] = sum(1 for c in comps if len(c) > 1)
        sim.conflict_order = conflict_order(cmds, views[0], ran)
    return sim, mc, bad, census


def run_gpu_case(wire, n, seed, fifo, env=None):
    """n GpuNodes beside a ModelCluster: the differential check run by run, then the states, then every end-of-run check on the
    contexts' own state -> (census, every frame every node emitted)"""
    cmds = Commands()
    gc, mc = GpuCluster(wire, n, cmds, env), ModelCluster(n, cmds)
    try:
        sim = Simulation(n, seed, fifo, gc, shadow=mc, cmds=cmds)
        sim.run()
        led = sorted(sim.led_at)
        tag = "n=%d seed=%d fifo=%s" % (n, seed, fifo)
        for r in range(n):
            got, want = gc.state(r, led), mc.state(r, led)
            for inst in led:
                assert got[0][inst] == want[0][inst], (tag, "replica", r, inst, got[0][inst], want[0][inst])
            assert got[1:] == want[1:], (tag, "replica", r, got[1:], want[1:])
        # ---- from here on the contexts' own state alone
        views = [gc.view(r, led) for r in range(n)]
        bad = check_invariants(n, cmds, views, sim.proposed, led)
        assert not bad, (tag, bad[:5])
        for r, node in enumerate(gc.nodes):
            node.check_store()
            assert node.carried == sim.carried[r]
        census = {k: int(sim.census[k]) for k in CENSUS_KEYS}
        assert census["deferred_reply"] == sum(node.deferred for node in gc.nodes), tag
        runs = []
        for r, node in enumerate(gc.nodes):
            insts, leader, number, deps, ends, first, count = execution_arrays(n, views[r])
            order, comp, ncomp, needs_host = node.epx.execute(leader, number, deps, first, count, deps_values_end=ends)
            assert needs_host == 0, (tag, r)
            ran = check_execution(n, cmds, views[r], order, comp)
            assert ncomp == len(set(int(c) for c in comp))
            runs.append((ran, [int(c) for c in comp], conflict_order(cmds, views[r], ran)))
        assert all(x == runs[0] for x in runs), (tag, "the replicas execute differently")
        sizes = collections.Counter(runs[0][1])
        census["exec_cycle"] = sum(1 for c in sizes.values() if c > 1)
        return census, [list(node.sent) for node in gc.nodes]
    finally:
        gc.close()


# ---- the committed cases: (n, seed, fifo) -> the census the model alone gives (tests/test_epaxos_cluster_cpu.py) -----------------
CASES = {
    (3, 3, True): {'fast_commit': 119, 'slow_disagreement': 0, 'slow_timer': 0, 'slow_commit': 1, 'nack_at_leader': 0, 'back_to_pre_accept': 0, 'back_to_accept': 0, 'back_to_prepare': 14, 'ok_status_0': 0, 'ok_status_2': 4, 'ok_status_3': 0, 'decide_noop': 0, 'decide_pre_accept': 0, 'decide_accept_accepted': 0, 'decide_accept_popular': 1, 'recovery_races_leader': 3, 'reply_after_decision': 81, 'commit_and_prepare_one_burst': 2, 'deferred_reply': 7, 'mk_fast': 19, 'mk_slow': 0, 'mk_recovered': 0, 'mk_reply': 6, 'burst_over_64_replica': 1, 'burst_over_64_leader': 1, 'exec_cycle': 1},
    (3, 4, False): {'fast_commit': 114, 'slow_disagreement': 0, 'slow_timer': 0, 'slow_commit': 6, 'nack_at_leader': 6, 'back_to_pre_accept': 44, 'back_to_accept': 1, 'back_to_prepare': 49, 'ok_status_0': 2, 'ok_status_2': 7, 'ok_status_3': 6, 'decide_noop': 0, 'decide_pre_accept': 1, 'decide_accept_accepted': 2, 'decide_accept_popular': 5, 'recovery_races_leader': 5, 'reply_after_decision': 78, 'commit_and_prepare_one_burst': 3, 'deferred_reply': 21, 'mk_fast': 19, 'mk_slow': 1, 'mk_recovered': 5, 'mk_reply': 18, 'burst_over_64_replica': 2, 'burst_over_64_leader': 0, 'exec_cycle': 4},
    (3, 22, False): {'fast_commit': 116, 'slow_disagreement': 0, 'slow_timer': 0, 'slow_commit': 4, 'nack_at_leader': 6, 'back_to_pre_accept': 30, 'back_to_accept': 5, 'back_to_prepare': 14, 'ok_status_0': 2, 'ok_status_2': 7, 'ok_status_3': 1, 'decide_noop': 1, 'decide_pre_accept': 0, 'decide_accept_accepted': 0, 'decide_accept_popular': 4, 'recovery_races_leader': 4, 'reply_after_decision': 32, 'commit_and_prepare_one_burst': 1, 'deferred_reply': 8, 'mk_fast': 24, 'mk_slow': 0, 'mk_recovered': 0, 'mk_reply': 7, 'burst_over_64_replica': 0, 'burst_over_64_leader': 1, 'exec_cycle': 3},
    (3, 22, True): {'fast_commit': 113, 'slow_disagreement': 0, 'slow_timer': 0, 'slow_commit': 9, 'nack_at_leader': 11, 'back_to_pre_accept': 33, 'back_to_accept': 4, 'back_to_prepare': 90, 'ok_status_0': 4, 'ok_status_2': 13, 'ok_status_3': 1, 'decide_noop': 3, 'decide_pre_accept': 1, 'decide_accept_accepted': 1, 'decide_accept_popular': 5, 'recovery_races_leader': 5, 'reply_after_decision': 95, 'commit_and_prepare_one_burst': 0, 'deferred_reply': 41, 'mk_fast': 19, 'mk_slow': 1, 'mk_recovered': 1, 'mk_reply': 21, 'burst_over_64_replica': 2, 'burst_over_64_leader': 0, 'exec_cycle': 4},
    (5, 6, False): {'fast_commit': 42, 'slow_disagreement': 96, 'slow_timer': 36, 'slow_commit': 158, 'nack_at_leader': 58, 'back_to_pre_accept': 22, 'back_to_accept': 92, 'back_to_prepare': 267, 'ok_status_0': 22, 'ok_status_2': 96, 'ok_status_3': 62, 'decide_noop': 1, 'decide_pre_accept': 16, 'decide_accept_accepted': 13, 'decide_accept_popular': 11, 'recovery_races_leader': 36, 'reply_after_decision': 437, 'commit_and_prepare_one_burst': 6, 'deferred_reply': 75, 'mk_fast': 2, 'mk_slow': 23, 'mk_recovered': 6, 'mk_reply': 73, 'burst_over_64_replica': 4, 'burst_over_64_leader': 1, 'exec_cycle': 6},
    (5, 8, True): {'fast_commit': 83, 'slow_disagreement': 46, 'slow_timer': 48, 'slow_commit': 122, 'nack_at_leader': 81, 'back_to_pre_accept': 33, 'back_to_accept': 31, 'back_to_prepare': 313, 'ok_status_0': 29, 'ok_status_2': 107, 'ok_status_3': 20, 'decide_noop': 1, 'decide_pre_accept': 15, 'decide_accept_accepted': 8, 'decide_accept_popular': 16, 'recovery_races_leader': 34, 'reply_after_decision': 422, 'commit_and_prepare_one_burst': 2, 'deferred_reply': 97, 'mk_fast': 10, 'mk_slow': 17, 'mk_recovered': 9, 'mk_reply': 86, 'burst_over_64_replica': 3, 'burst_over_64_leader': 1, 'exec_cycle': 2},
    (7, 30, True): {'fast_commit': 25, 'slow_disagreement': 65, 'slow_timer': 180, 'slow_commit': 267, 'nack_at_leader': 141, 'back_to_pre_accept': 45, 'back_to_accept': 84, 'back_to_prepare': 1006, 'ok_status_0': 35, 'ok_status_2': 94, 'ok_status_3': 273, 'decide_noop': 1, 'decide_pre_accept': 11, 'decide_accept_accepted': 39, 'decide_accept_popular': 5, 'recovery_races_leader': 44, 'reply_after_decision': 1256, 'commit_and_prepare_one_burst': 3, 'deferred_reply': 171, 'mk_fast': 1, 'mk_slow': 49, 'mk_recovered': 12, 'mk_reply': 280, 'burst_over_64_replica': 4, 'burst_over_64_leader': 1, 'exec_cycle': 1},
    (7, 112, False): {'fast_commit': 22, 'slow_disagreement': 104, 'slow_timer': 143, 'slow_commit': 258, 'nack_at_leader': 36, 'back_to_pre_accept': 64, 'back_to_accept': 240, 'back_to_prepare': 792, 'ok_status_0': 17, 'ok_status_2': 68, 'ok_status_3': 108, 'decide_noop': 1, 'decide_pre_accept': 6, 'decide_accept_accepted': 13, 'decide_accept_popular': 4, 'recovery_races_leader': 18, 'reply_after_decision': 907, 'commit_and_prepare_one_burst': 8, 'deferred_reply': 84, 'mk_fast': 1, 'mk_slow': 43, 'mk_recovered': 5, 'mk_reply': 190, 'burst_over_64_replica': 12, 'burst_over_64_leader': 2, 'exec_cycle': 5},
}
OTHER_FORM_CASES = [(3, 22, True), (5, 8, True), (7, 30, True)]
REFERENCE_RECOVERY_CASE = (3, 1, True)
SEEN_NOWHERE = set()                # classes of the census that no committed seed reaches at any n
