"""The node-message unwrap (csrc/wire_unwrap.h) and the BATCH splitter
(_hostpack.gather_node_texts) restated in Python, and the corpus the node-wire tests share.

unwrap(text, esc) -> (class, unwrapped bytes of len(text)); split(entry) -> the member
bodies (still escaped) of a strictly parsed BATCH, or None; gather(entries) -> what
gather_node_texts returns, as Python lists.  The rules are DESIGN.md "Node messages".
tests/test_wire_unwrap.py holds this against batching.requests_in_drain and json.loads,
and the C++ twin and the extension against this.
"""
import json
import random
import re

import wire_model
from wire_model import MAX_DIGITS, MAX_MEMBERS, MAX_TEXT

REQUEST, HOST, NONE = 0, 1, 2

_WS = b" \t\n\r"
_DELIM = b" \t\n\r,}]"
_UNESC = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13,
          ord("t"): 9}
_INT = re.compile(rb"-?(?:0|[1-9][0-9]*)")
_STRICT_STRING = re.compile(rb'"(?:[\x20\x21\x23-\x5b\x5d-\x7f]|\\["\\/bfnrt])*"')


class _Host(Exception):
    pass


def _ws(t, p, m):
    while p < m and t[p] in _WS:
        p += 1
    return p


def _skip_string(t, p, m):
    """ws_skip_string: lenient, a backslash hides the next byte."""
    p += 1
    while p < m:
        if t[p] == 0x22:
            return p + 1
        p += 2 if t[p] == 0x5C else 1
    raise _Host


def _skip_value(t, p, m):
    """ws_skip_value: structure only (brackets counted whatever their kind)."""
    c = t[p]
    if c == 0x22:
        return _skip_string(t, p, m)
    if c in b"{[":
        depth = 0
        while p < m:
            c = t[p]
            if c == 0x22:
                p = _skip_string(t, p, m)
                continue
            if c in b"{[":
                depth += 1
            if c in b"}]":
                depth -= 1
                if depth == 0:
                    return p + 1
            p += 1
        raise _Host
    s = p
    while p < m and t[p] not in _DELIM:
        p += 1
    if p == s:
        raise _Host
    return p


def _strict_scalar(v):
    """wu_scalar: the bytes v are exactly one scalar of the scanner's grammar."""
    if v[:1] == b'"':
        return _STRICT_STRING.fullmatch(v) is not None
    if v in (b"true", b"false", b"null"):
        return True
    return _INT.fullmatch(v) is not None and len(v.lstrip(b"-")) <= MAX_DIGITS and v != b"-0"


def _members(t, p, m):
    """wu_walk: [(key bytes, value start, value end)], the position after '}'."""
    out = []
    q = _ws(t, p + 1, m)
    if q >= m:
        raise _Host
    if t[q] == 0x7D:
        return out, q + 1
    while True:
        q = _ws(t, q, m)
        if q >= m or t[q] != 0x22 or len(out) == MAX_MEMBERS:
            raise _Host
        k = q + 1
        q = k
        while True:
            if q >= m:
                raise _Host
            c = t[q]
            if c == 0x22:
                break
            if c == 0x5C or c < 0x20 or c >= 0x80:
                raise _Host
            q += 1
        key = bytes(t[k:q])
        q = _ws(t, q + 1, m)
        if q >= m or t[q] != 0x3A:
            raise _Host
        q = _ws(t, q + 1, m)
        if q >= m:
            raise _Host
        v = q
        q = _skip_value(t, q, m)
        out.append((key, v, q))
        q = _ws(t, q, m)
        if q >= m:
            raise _Host
        d = t[q]
        q += 1
        if d == 0x7D:
            return out, q
        if d != 0x2C:
            raise _Host


def _one(members, name):
    """The (start, end) of the one member `name`, None without one; two -> host."""
    found = [(v, e) for k, v, e in members if k == name]
    if len(found) > 1:
        raise _Host
    return found[0] if found else None


def _first_special(members):
    """wu_walk meets a second op / request / signature as it goes: the members up to there
    must have parsed, which _members has already seen to; so only the count matters."""
    for name in (b"op", b"request", b"signature"):
        _one(members, name)


def unwrap(text, esc):
    n = len(text)
    blank = b" " * n
    if n > MAX_TEXT:
        return HOST, blank
    try:
        if esc:
            buf, p = bytearray(), 0
            while p < n:
                c = text[p]
                if c < 0x20 or c > 0x7E:
                    raise _Host
                if c == 0x5C:
                    p += 1
                    c = _UNESC.get(text[p]) if p < n else None
                    if c is None:
                        raise _Host
                buf.append(c)
                p += 1
            t = bytes(buf)
        else:
            t = bytes(text)
        m = len(t)
        p = _ws(t, 0, m)
        if p >= m or t[p] != 0x7B:
            raise _Host
        members, end = _members(t, p, m)
        _first_special(members)
        if _ws(t, end, m) != m:
            raise _Host
        op = _one(members, b"op")
        kind = None
        if op is not None and t[op[0]] == 0x22:
            value = t[op[0] + 1:op[1] - 1]
            if b"\\" in value:
                raise _Host
            kind = value
        if kind == b"BATCH":
            raise _Host
        if kind != b"PROPAGATE":
            if _one(members, b"signature") is None:
                return NONE, blank
            a, b = p, end
        else:
            req = _one(members, b"request")
            if req is None or t[req[0]] != 0x7B:
                return NONE, blank
            inner, inner_end = _members(t, req[0], req[1])
            _first_special(inner)
            if inner_end != req[1]:
                raise _Host
            if _one(inner, b"signature") is None:
                return NONE, blank
            for _, v, e in members:
                if v != req[0] and not _strict_scalar(t[v:e]):
                    raise _Host
            a, b = req
    except _Host:
        return HOST, blank
    return REQUEST, b" " * a + t[a:b] + b" " * (n - b)


# ------------------------------------------------------------------ the splitter
_SP = rb"[ \t\n\r]*"
_MEMBER = rb'"((?:[^"\\]|\\["\\/bfnrt])*)"'
_LATER_VALUE = rb'(?:null|true|false|-?(?:0|[1-9][0-9]{0,17})|"[^"\\]*")'
_BATCH = re.compile(
    _SP + rb"\{" + _SP + rb'"op"' + _SP + rb":" + _SP + rb'"BATCH"' + _SP + rb"," + _SP + rb'"messages"' + _SP + rb":"
    + _SP + rb"\[" + _SP + rb"((?:" + _MEMBER + rb"(?:" + _SP + rb"," + _SP + _MEMBER + rb")*)?)" + _SP + rb"\]"
    + rb"((?:" + _SP + rb"," + _SP + rb'"[^"\\]*"' + _SP + rb":" + _SP + _LATER_VALUE + rb")*)" + _SP + rb"\}" + _SP)
_LATER_KEY = re.compile(rb"," + _SP + rb'"([^"\\]*)"' + _SP + rb":" + _SP + _LATER_VALUE)


def split(entry):
    """The still-escaped bodies of the BATCH's member strings, or None: not split."""
    if any(c < 0x20 or c > 0x7E for c in entry):
        return None
    mt = _BATCH.fullmatch(entry)
    if mt is None:
        return None
    rest, keys = mt.group(4), []
    pos = 0
    while True:  # the later members again, one at a time (-0 and "op" / "messages" are refused)
        pos = _ws(rest, pos, len(rest))
        if pos >= len(rest):
            break
        km = _LATER_KEY.match(rest, pos)
        keys.append(km.group(1))
        if km.group(0).rstrip().endswith(b"-0"):
            return None
        pos = km.end()
    if b"op" in keys or b"messages" in keys:
        return None
    return [bytes(x.group(1)) for x in re.finditer(_MEMBER, mt.group(1))]


def gather(entries):
    """(bodies back to back, off[m + 1], esc[m], entry[m])."""
    parts, esc, entry = [], [], []
    for e, raw in enumerate(entries):
        bodies = split(raw)
        if bodies is None:
            parts.append(raw)
            esc.append(0)
            entry.append(e)
        else:
            parts += bodies
            esc += [1] * len(bodies)
            entry += [e] * len(bodies)
    off = [0]
    for b in parts:
        off.append(off[-1] + len(b))
    return b"".join(parts), off, esc, entry


# ------------------------------------------------------------------ the corpus
def _dumps(r, d):
    return json.dumps(d, separators=r.choice([(",", ":"), (", ", ": ")]))


def _spaced(text):
    """Whitespace at every token boundary of a JSON text."""
    out, in_str, skip = [], False, False
    for ch in text:
        if in_str:
            out.append(ch)
            if skip:
                skip = False
            elif ch == "\\":
                skip = True
            elif ch == '"':
                in_str = False
                out.append(" \n")
            continue
        if ch == '"':
            in_str = True
            out.append(" " + ch)
        elif ch in "{}[],:":
            out.append("\t " + ch + " \r")
        else:
            out.append(ch)
    return "".join(out)


_CORPUS = {}


def corpus():
    """{"clean": [entry bytes, ...], "mutated": [...]} (fixed seed, built once).

    clean: straight json.dumps output over ASCII NYM requests -- bare requests, PROPAGATEs
    (nodeloop.propagate_text) and BATCHes (nodeloop.batch_text) of 0, 1, 2 and 70 members mixing
    PROPAGATEs with PREPARE-like dicts.  mutated: the variations the unwrap and the splitter
    must class or decline."""
    if _CORPUS:
        return _CORPUS
    from plenum_amd.nodeloop import batch_text, propagate_text
    r = random.Random(20241020)
    reqs = [wire_model.nym_dict(r, i) for i in range(90)]
    req_texts = [_dumps(r, d) for d in reqs]
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(reqs)]
    prepares = [json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": i, "ppTime": 1_600_000_000 + i,
                            "digest": "d%032x" % r.getrandbits(128), "stateRootHash": None, "txnRootHash": None})
                for i in range(8)]

    def mix(k):
        return [props[j] if j % 5 else prepares[j % 8] for j in range(k)]

    batches = [batch_text(mix(k)) for k in (0, 1, 2, 70)] + [batch_text([req_texts[3], props[4]])]
    clean = [t.encode() for t in req_texts[:20] + props[:20] + prepares[:3] + batches]

    p0, q0, b2 = props[0], req_texts[0], batches[2]
    req0 = json.dumps(reqs[0])
    no_sig = {k: v for k, v in reqs[1].items() if k != "signature"}
    mut = []
    mut += [_spaced(t) for t in (q0, p0, b2, batches[1])]
    mut += [json.dumps({"request": reqs[0], "op": "PROPAGATE", "senderClient": "c"}),       # op not first
            json.dumps({"messages": [p0], "op": "BATCH", "signature": None}),
            json.dumps({"op": 7, "request": reqs[0], "senderClient": "c"}),                   # op a number
            json.dumps({"op": 7, "signature": "x", "identifier": "i"}),
            p0[:-1] + ', "op": "PROPAGATE"}', p0[:-1] + ', "op": "X"}',                        # duplicates
            p0[:-1] + ', "request": {}}', p0[:-1] + ', "signature": 1, "signature": 2}',
            q0[:-1] + ', "signature": "x"}', q0[:-1] + ', "op": 1, "op": 2}',
            '{"op": "PROPAGATE", "request": %s, "senderClient": "c"}' % (req0[:-1] + ', "signature": "z"}'),
            json.dumps({"op": "PROPAGATE", "request": [reqs[0]], "senderClient": "c"}),      # request a list
            json.dumps({"op": "PROPAGATE", "request": req0, "senderClient": "c"}),           # ... a string
            json.dumps({"op": "PROPAGATE", "senderClient": "c"}),
            propagate_text(no_sig, "c"), json.dumps(no_sig),                                 # no signature
            json.dumps({"op": "PROPAGATE", "request": reqs[0], "senderClient": {"a": 1}}),   # envelope values
            json.dumps({"op": "PROPAGATE", "request": reqs[0], "senderClient": 1.5}),
            json.dumps({"op": "PROPAGATE", "request": reqs[0], "senderClient": None, "n": -12, "t": True}),
            json.dumps({"op": "PROPAGATE", "request": reqs[0], "senderClient": 'q"\\/\n\t'}),
            p0.replace('"PROPAGATE"', '"PROP\\u0041GATE"'), p0.replace('"op"', '"o\\u0070"'),  # \u escapes
            p0.replace('"senderClient"', '"sender\\u0043lient"'), p0.replace("client0", "client\\u0030"),
            p0.replace('"request"', '"re\\u0071uest"'), p0.replace('"signature"', '"sign\\u0061ture"'),
            q0.replace('"signature"', '"sign\\u0061ture"'), q0.replace('"reqId"', '"req\\u0049d"'),
            p0.replace("client0", "client\\x"), p0.replace("client0", "client\\"),
            batch_text([p0.replace("client0", "client\\u0030"), props[1]]),
            batch_text([batches[2], props[2]]), batch_text([batch_text([batch_text([props[5]])])]),  # nested
            json.dumps({"op": "BATCH", "messages": [p0, 5, None, {"a": 1}], "signature": None}),  # non-string member
            json.dumps({"op": "BATCH", "messages": p0, "signature": None}),
            json.dumps({"op": "BATCH", "messages": [p0], "signature": None, "n": 12, "t": True, "s": "x y"}),
            json.dumps({"op": "BATCH", "messages": [p0], "signature": {"a": 1}}),
            json.dumps({"op": "BATCH", "messages": [p0], "signature": 1.5}),
            json.dumps({"op": "BATCH", "messages": [p0], "n": 10**18}),
            '{"op":"BATCH","messages":[%s],"n":-0}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s],"n":01}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s],"op":1}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s],"messages":[]}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s],"k\\n":1}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s],"k":"a\\nb"}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s,]}' % json.dumps(p0), '{"op":"BATCH","messages":[,%s]}' % json.dumps(p0),
            '{"op":"BATCH","messages":[%s]x,"signature":null}' % json.dumps(p0),               # garbage after ]
            b2 + "x", b2 + "  \n", b2 + " ", p0 + "}", p0 + " x", q0 + "]", q0 + " \t",       # ... after }
            b2.replace("]", "],", 1), batch_text(["{}", "[]", "", " ", '"s"', "7", props[6][:40]]),
            batch_text([p0.replace("client0", "tab\there"), "\b" + props[7], props[8] + "\n", "café"]),
            batch_text([p0.replace("client0", "sl/ash\\back")]),
            "[%s]" % p0, json.dumps(p0), "", " ", "{", "{}", " {} ", "nul", "7"]
    mut = [t.encode() for t in mut]
    for raw in (b"\x01", b"\x7f", b"\xc3\xa9"):                                               # raw bytes
        mut += [p0.replace("client0", "cli%sent").encode() % raw, q0.replace('"reqId"', '"req%sId"').encode() % raw,
                b2.encode().replace(b"PROPAGATE", b"PROPA%sGATE" % raw, 1), raw + p0.encode(), b2.encode() + raw]
    for t in (q0, p0, b2, batches[1]):                                                        # truncations
        mut += [t.encode()[:k] for k in range(0, len(t), 7)]
    pad = json.dumps({"op": "PROPAGATE", "request": reqs[0], "senderClient": ""})
    for total in (4095, 4096, 4097):                                                          # the length limit
        mut.append(json.dumps({"op": "PROPAGATE", "request": reqs[0],
                               "senderClient": "x" * (total - len(pad))}).encode())
    long_member = mut[-1].decode()
    assert len(long_member) == 4097
    mut.append(batch_text([props[9], long_member, props[10]]).encode())                       # a member of 4,097 bytes
    for members in (32, 33):                                                                  # the member limit
        extra = {"k%02d" % j: j for j in range(members - 3)}
        mut.append(json.dumps(dict({"op": "PROPAGATE", "request": reqs[0], "senderClient": "c"}, **extra)).encode())
        mut.append(json.dumps(dict(reqs[0], **{"k%02d" % j: j for j in range(members - len(reqs[0]))})).encode())
    for t in r.choices(clean, k=60):                                                          # byte mutations
        mut.append(wire_model._mutate(r, t))
    _CORPUS.update(clean=clean, mutated=mut)
    return _CORPUS


def messages(entries):
    """Every message of the entries as gather() cuts them: [(body, esc)]."""
    buf, off, esc, _ = gather(entries)
    return [(buf[off[i]:off[i + 1]], esc[i]) for i in range(len(esc))]


# ------------------------------------------------------------------ the CPU twin
def twin_unwrap(lib, buf, off, esc):
    """libedv_hostcheck.so hc_wire_unwrap over packed messages: (cls[n], unwrapped bytes)."""
    import ctypes

    import numpy as np
    n = len(off) - 1
    buf = np.ascontiguousarray(buf, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    esc = np.ascontiguousarray(esc, np.uint8)
    cls = np.zeros(n, np.uint8)
    out = np.zeros(max(1, int(off[-1] - off[0])), np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.hc_wire_unwrap.restype = None
    lib.hc_wire_unwrap(P(buf), P(off), P(esc), ctypes.c_uint64(n), P(cls), P(out))
    return cls, out[:int(off[-1] - off[0])]
