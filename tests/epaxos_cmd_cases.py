"""TEST INFRASTRUCTURE: serialised CommandOrNoop messages (epaxos/EPaxos.proto:61-89 around statemachine/KeyValueStore.proto:
12-45) assembled by hand, and the key-list parser of csrc/fpx_epx_cmd_parse.hpp written a SECOND time, in Python, from the
rules in include/fpx_wire.h: what tests/test_epaxos_cmd_parse_cpu.py holds the host classify against, and what the GPU tests
of the classify and the replica tick build their frames and expectations from."""
import itertools
import random

from tests.epaxos_wire_cases import i32, ld, tag, varint

KEY_MAX_LEN = 4096
MALFORMED = "malformed"


# ---- building ---------------------------------------------------------------------------------------------------------
def get_request(keys):
    return ld(1, b"".join(ld(1, k) for k in keys))


def set_request(keys, value=b"v"):
    return ld(2, b"".join(ld(1, ld(1, k) + ld(2, value)) for k in keys))


def command_fields(body, address=b"\x0a\x00\x00\x01", pseudonym=3, client_id=7):
    """the four fields of a Command, in field order"""
    return [ld(1, address), i32(2, pseudonym), i32(3, client_id), ld(4, body)]


def command(body, order=(0, 1, 2, 3), **kw):
    f = command_fields(body, **kw)
    return ld(1, b"".join(f[j] for j in order))


def get(keys, **kw):
    return command(get_request(keys), **kw)


def set_(keys, **kw):
    return command(set_request(keys), **kw)


NOOP = ld(2, b"")


# ---- the parser, a second time -------------------------------------------------------------------------------------------
class Malformed(Exception):
    pass


def _varint(b, p, end):
    v = 0
    for shift in range(0, 70, 7):
        if p >= end:
            raise Malformed
        x = b[p]
        p += 1
        if shift < 64:
            v |= (x & 0x7f) << shift
        if not x & 0x80:
            return v & ((1 << 64) - 1), p
    raise Malformed


def _fields(b, p, end):
    """(field, wire type, value or (start, end)) of every field of b[p:end]"""
    while p < end:
        t, p = _varint(b, p, end)
        field, wt = (t >> 3) & 0xffffffff, t & 7        # (the readers of csrc keep 32 bits of a field number)
        if wt == 0:
            v, p = _varint(b, p, end)
            yield field, wt, v
        elif wt == 1 or wt == 5:
            n = 8 if wt == 1 else 4
            if end - p < n:
                raise Malformed
            yield field, wt, None
            p += n
        elif wt == 2:
            n, p = _varint(b, p, end)
            if n > end - p:
                raise Malformed
            yield field, wt, (p, p + n)
            p += n
        else:
            raise Malformed


def parse_command(b):
    """MALFORMED, or (shape, is_noop, is_set, keys): the rules of include/fpx_wire.h.  Every occurrence of a known
    length-delimited field is walked down to the keys, so a frame is malformed whatever its shape"""
    b = bytes(b)
    odd = False
    commands = noops = requests = 0
    is_set = 0
    keys = []
    try:
        for f, wt, v in _fields(b, 0, len(b)):
            if f == 1 and wt == 2:
                commands += 1
                seen, bodies = set(), 0
                for cf, cwt, cv in _fields(b, *v):
                    if cf == 4 and cwt == 2:
                        bodies += 1
                        for rf, rwt, rv in _fields(b, *cv):
                            if rf in (1, 2) and rwt == 2:
                                requests += 1
                                is_set = int(rf == 2)
                                for kf, kwt, kv in _fields(b, *rv):
                                    if kf != 1 or kwt != 2:
                                        odd = True
                                    elif rf == 1:
                                        keys.append(b[kv[0]:kv[1]])
                                    else:
                                        nkey = nvalue = 0
                                        for pf, pwt, pv in _fields(b, *kv):
                                            if pf == 1 and pwt == 2:
                                                nkey += 1
                                                if nkey == 1:
                                                    keys.append(b[pv[0]:pv[1]])
                                            elif pf == 2 and pwt == 2:
                                                nvalue += 1
                                            else:
                                                odd = True
                                        if nkey != 1 or nvalue < 1:
                                            odd = True
                            else:
                                odd = True
                    elif (cf == 1 and cwt == 2) or (cf in (2, 3) and cwt == 0):
                        pass
                    else:
                        odd = True
                        continue
                    seen.add(cf)
                if seen != {1, 2, 3, 4} or bodies != 1:
                    odd = True
            elif f == 2 and wt == 2:
                noops += 1
                if v[1] != v[0]:
                    odd = True
            else:
                odd = True
    except Malformed:
        return MALFORMED
    if any(len(k) > KEY_MAX_LEN for k in keys):
        odd = True
    noop = commands == 0 and noops == 1
    cmd = commands == 1 and noops == 0 and requests == 1
    if odd or not (noop or cmd):
        return (0, 0, 0, [])
    return (1, int(noop), is_set if cmd else 0, keys)


def classify(cmds):
    """what fpx_wire_epx_classify returns for the serialised commands (None = the message has none): a dict, or
    (MALFORMED, index) for the first malformed one"""
    out = {"key_offsets": [0], "keys": [], "is_set": [], "is_noop": [], "cmd_shape": []}
    bad = None
    for i, c in enumerate(cmds):
        r = (-1, -1, 0, []) if c is None else parse_command(c)
        if r == MALFORMED:
            bad = i if bad is None else bad
            r = (0, 0, 0, [])
        shape, noop, is_set, keys = r
        out["keys"] += keys
        out["key_offsets"].append(len(out["keys"]))
        out["is_set"].append(is_set), out["is_noop"].append(noop), out["cmd_shape"].append(shape)
    return (MALFORMED, bad) if bad is not None else out


class KeyDict:
    """the key table as a dict filled in first-occurrence order"""

    def __init__(self):
        self.ids = {}

    def intern(self, keys):
        return [self.ids.setdefault(bytes(k), len(self.ids)) for k in keys]

    def order(self):
        return list(self.ids)


# ---- cases: (name, bytes, expected) -----------------------------------------------------------------------------------------
def edge_cases():
    long_ok, long_bad = b"x" * KEY_MAX_LEN, b"y" * (KEY_MAX_LEN + 1)
    five = [b"k%d" % j for j in range(5)]
    body = get_request([b"a"])
    f = command_fields(body)
    cases = [
        ("noop", NOOP, (1, 1, 0, [])),
        ("get 0", get([]), (1, 0, 0, [])),
        ("get 1", get([b"a"]), (1, 0, 0, [b"a"])),
        ("get 5", get(five), (1, 0, 0, five)),
        ("set 1", set_([b"a"]), (1, 0, 1, [b"a"])),
        ("set 3", set_([b"a", b"bb", b"c"]), (1, 0, 1, [b"a", b"bb", b"c"])),
        ("a key twice", get([b"a", b"b", b"a"]), (1, 0, 0, [b"a", b"b", b"a"])),
        ("the empty key", get([b""]), (1, 0, 0, [b""])),
        ("the empty key in a set", set_([b"", b"a"]), (1, 0, 1, [b"", b"a"])),
        ("a 4096-byte key", get([long_ok, b"a"]), (1, 0, 0, [long_ok, b"a"])),
        ("a 4097-byte key", get([long_bad]), (0, 0, 0, [])),
        ("a 4097-byte key in a set", set_([b"a", long_bad]), (0, 0, 0, [])),
        ("a set request without pairs", command(ld(2, b"")), (1, 0, 1, [])),
        ("command before client_address", command(body, order=(3, 0, 1, 2)), (1, 0, 0, [b"a"])),
        ("command after client_address", command(body, order=(0, 3, 1, 2)), (1, 0, 0, [b"a"])),
        ("client_id twice", ld(1, b"".join(f) + f[2]), (1, 0, 0, [b"a"])),
        # shape 0
        ("both request members", command(get_request([b"a"]) + set_request([b"b"])), (0, 0, 0, [])),
        ("a member twice", command(get_request([b"a"]) + get_request([b"b"])), (0, 0, 0, [])),
        ("command twice", ld(1, b"".join(f) + f[3]), (0, 0, 0, [])),
        ("two Commands", get([b"a"]) + get([b"b"]), (0, 0, 0, [])),
        ("a Command and a Noop", get([b"a"]) + NOOP, (0, 0, 0, [])),
        ("two Noops", NOOP + NOOP, (0, 0, 0, [])),
        ("a pair with two keys", command(ld(2, ld(1, ld(1, b"a") + ld(1, b"b") + ld(2, b"v")))), (0, 0, 0, [])),
        ("a pair without a key", command(ld(2, ld(1, ld(2, b"v")))), (0, 0, 0, [])),
        ("a pair without a value", command(ld(2, ld(1, ld(1, b"a")))), (0, 0, 0, [])),
        ("unknown field in CommandOrNoop", get([b"a"]) + i32(9, 1), (0, 0, 0, [])),
        ("unknown field in Command", ld(1, b"".join(f) + i32(9, 1)), (0, 0, 0, [])),
        ("unknown field in KeyValueStoreInput", command(body + ld(7, b"zz")), (0, 0, 0, [])),
        ("unknown field in GetRequest", command(ld(1, ld(1, b"a") + i32(2, 5))), (0, 0, 0, [])),
        ("unknown field in SetRequest", command(ld(2, ld(1, ld(1, b"a") + ld(2, b"v")) + i32(3, 1))), (0, 0, 0, [])),
        ("unknown field in a pair", command(ld(2, ld(1, ld(1, b"a") + ld(2, b"v") + tag(5, 5) + b"abcd"))), (0, 0, 0, [])),
        ("a body in Noop", ld(2, i32(1, 1)), (0, 0, 0, [])),
        ("Request.Empty", command(b""), (0, 0, 0, [])),
        ("an empty CommandOrNoop", b"", (0, 0, 0, [])),
        ("client_id missing", ld(1, f[0] + f[1] + f[3]), (0, 0, 0, [])),
        ("command as a varint", ld(1, f[0] + f[1] + f[2] + i32(4, 1)), (0, 0, 0, [])),
        # malformed
        ("a key running past its request", command(ld(1, tag(1, 2) + varint(9) + b"ab")), MALFORMED),
        ("a group", get([b"a"]) + tag(3, 3), MALFORMED),
        ("an unfinished varint", get([b"a"]) + b"\x88\x80", MALFORMED),
        ("a malformed second Command", get([b"a"]) + ld(1, tag(4, 2) + varint(3) + b"a"), MALFORMED),
        ("a fixed32 cut short", get([b"a"]) + tag(6, 5) + b"ab", MALFORMED),
    ]
    for order in itertools.permutations(range(4)):
        cases.append(("Command fields in order %s" % (order,), command(body, order=order), (1, 0, 0, [b"a"])))
    return cases


def truncations(msg=None):
    """every proper prefix of one canonical message: none may stay canonical"""
    msg = set_([b"alpha", b"", b"k7"]) if msg is None else msg
    return [msg[:j] for j in range(len(msg))]


def random_command(rng, keys=None):
    """a canonical command mostly; now and then one of the odd shapes or a mutation"""
    pool = keys or [b"k%d" % j for j in range(12)] + [b"", b"a" * 300]
    r = rng.random()
    if r < 0.1:
        return NOOP
    ks = [rng.choice(pool) for _ in range(rng.choice((0, 1, 1, 1, 2, 3, 5)))]
    order = tuple(rng.sample(range(4), 4))
    msg = (set_ if rng.random() < 0.5 else get)(ks, order=order, client_id=rng.randrange(1 << 20))
    if r > 0.85:
        b = bytearray(msg)
        how = rng.randrange(3)
        if how == 0 and b:
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif how == 1:
            b = b[:rng.randrange(len(b) + 1)]
        else:
            b += rng.choice((i32(9, 4), NOOP, ld(1, b"")))
        msg = bytes(b)
    return msg


def seeded_burst(seed, m):
    rng = random.Random(seed)
    return [None if rng.random() < 0.05 else random_command(rng) for _ in range(m)]
