"""The wire scanner's grammar restated in Python, and the corpus the wire tests share.

scan(text) -> (serialization bytes, identifier, signature text), or None where the
text is outside the GPU grammar (csrc/wire_scan.h: "the host decides").  The rules
are the ones DESIGN.md "Wire scan" lists; this restatement is recursive and builds
Python objects, the scanner is iterative over bytes -- tests/test_wire_scan.py holds
the two against each other and this one against json.loads + plenum_amd.serialization.
"""
import json
import random
import re

MAX_TEXT = 4096
MAX_DEPTH = 8
MAX_MEMBERS = 32
MAX_DIGITS = 18
MAX_SIG_CHARS = 95
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"

_WS = b" \t\n\r"
_DELIM = b" \t\n\r,}]"
_ESC = {ord('"'): '"', ord("\\"): "\\", ord("/"): "/", ord("b"): "\b", ord("f"): "\f", ord("n"): "\n",
        ord("r"): "\r", ord("t"): "\t"}
_INT = re.compile(rb"-?(?:0|[1-9][0-9]*)")
_LITERALS = ((b"true", "True"), (b"false", "False"), (b"null", ""))


class _Host(Exception):
    pass


def _ws(t, p):
    while p < len(t) and t[p] in _WS:
        p += 1
    return p


def _need(t, p):
    if p >= len(t):
        raise _Host
    return t[p]


def _string(t, p):
    """The string opening at p: (text, position after it, whether it had an escape)."""
    out, esc = [], False
    p += 1
    while True:
        c = _need(t, p)
        if c == 0x22:
            return "".join(out), p + 1, esc
        if c < 0x20 or c >= 0x80:
            raise _Host
        if c == 0x5C:
            esc = True
            p += 1
            ch = _ESC.get(_need(t, p))
            if ch is None:
                raise _Host
            out.append(ch)
        else:
            out.append(chr(c))
        p += 1


def _scalar_end(t, p):
    if p >= len(t) or t[p] not in _DELIM:
        raise _Host
    return p


def _value(t, p, depth):
    """The value at p inside a container at `depth`: (signing text, position after it,
    (kind, had an escape))."""
    c = _need(t, p)
    if c == 0x7B:
        s, p = _object(t, p, depth + 1)
        return s, p, ("object", False)
    if c == 0x5B:
        if depth + 1 > MAX_DEPTH:
            raise _Host
        items = []
        p = _ws(t, p + 1)
        if _need(t, p) == 0x5D:
            return "", p + 1, ("array", False)
        while True:
            s, p, _ = _value(t, _ws(t, p), depth + 1)
            items.append(s)
            p = _ws(t, p)
            c = _need(t, p)
            p += 1
            if c == 0x5D:
                return ",".join(items), p, ("array", False)
            if c != 0x2C:
                raise _Host
    if c == 0x22:
        s, p, esc = _string(t, p)
        return s, p, ("string", esc)
    m = _INT.match(t, p)
    if m is not None:
        num = m.group()
        if len(num.lstrip(b"-")) > MAX_DIGITS or num == b"-0":
            raise _Host
        return num.decode(), _scalar_end(t, m.end()), ("number", False)
    for word, text in _LITERALS:
        if t.startswith(word, p):
            return text, _scalar_end(t, p + len(word)), ("literal", False)
    raise _Host


def _object(t, p, depth, top=None):
    """The object opening at p: (signing text, position after it).  top: a dict that
    receives the top-level identifier and signature, the latter left out of the text."""
    if depth > MAX_DEPTH:
        raise _Host
    members = {}
    p = _ws(t, p + 1)
    if _need(t, p) == 0x7D:
        if top is not None:
            raise _Host
        return "", p + 1
    while True:
        p = _ws(t, p)
        if _need(t, p) != 0x22:
            raise _Host
        key, p, esc = _string(t, p)
        if esc or key in members or len(members) == MAX_MEMBERS:
            raise _Host
        p = _ws(t, p)
        if _need(t, p) != 0x3A:
            raise _Host
        s, p, kind = _value(t, _ws(t, p + 1), depth)
        members[key] = s
        if top is not None and key in ("signature", "identifier"):
            if kind != ("string", False) or not s:
                raise _Host
            top[key] = s
        p = _ws(t, p)
        c = _need(t, p)
        p += 1
        if c == 0x7D:
            break
        if c != 0x2C:
            raise _Host
    names = sorted(k for k in members if top is None or k != "signature")
    return "|".join(k + ":" + members[k] for k in names), p


def scan(text):
    if len(text) > MAX_TEXT:
        return None
    try:
        p = _ws(text, 0)
        if _need(text, p) != 0x7B:
            raise _Host
        top = {}
        ser, p = _object(text, p, 1, top)
        if _ws(text, p) != len(text) or "signature" not in top or "identifier" not in top:
            raise _Host
        sig = top["signature"]
        if len(sig) > MAX_SIG_CHARS or any(ch not in B58 for ch in sig):
            raise _Host
    except _Host:
        return None
    return ser.encode("ascii"), top["identifier"], sig


# ------------------------------------------------------------------ the corpus
def b58(raw):
    v, out = int.from_bytes(raw, "big"), []
    while v:
        v, d = divmod(v, 58)
        out.append(B58[d])
    return "1" * (len(raw) - len(raw.lstrip(b"\0"))) + "".join(reversed(out))


def _rand_sig(r, nbytes=64, zeros=0):
    head = bytes([r.randrange(1, 256)])
    return b58(b"\0" * zeros + head + bytes(r.getrandbits(8) for _ in range(nbytes - zeros - 1)))


def _rand_scalar(r):
    k = r.randrange(16)
    if k < 4:
        return r.choice(["", "abc", "a|b:c,d", 'q"uo\\te/', "tab\there\n", "x" * r.randrange(40), "~AbC123", "\x7f"])
    if k < 8:
        return r.choice([0, 1, -1, 7, 10**17, 10**18 - 1, -(10**18 - 1), r.randrange(-10**12, 10**12)])
    if k < 10:
        return r.choice([True, False])
    if k < 12:
        return None
    if k == 12:
        return r.choice(["ключ", "é", "值"])  # non-ASCII: the host decides
    if k == 13:
        return r.choice([0.5, 1e16, -0.0, 1e-5, float("inf"), float("nan")])
    if k == 14:
        return r.choice([10**18, -10**18, 10**30])
    return r.choice(["\b\f\r", "\x01", " "])


def _rand_obj(r, depth=0):
    k = r.randrange(10)
    if depth > 4 or k < 5:
        return _rand_scalar(r)
    if k < 7:
        return [_rand_obj(r, depth + 1) for _ in range(r.randrange(5))]
    keys = ["".join(r.choice("abcXYZ_ 1") for _ in range(r.randrange(0, 5))) for _ in range(r.randrange(6))]
    return {k_: _rand_obj(r, depth + 1) for k_ in keys}


def nym_dict(r, i):
    """A request dict of plenum_amd.synth.nym_request's shape with a well-formed signature."""
    from plenum_amd.synth import nym_request
    d = nym_request(b58(bytes(r.getrandbits(8) for _ in range(16))), 1_500_000_000_000_000 + i,
                    b58(bytes(r.getrandbits(8) for _ in range(16))),
                    "~" + b58(bytes(r.getrandbits(8) for _ in range(16))), alias="al%d" % i if i % 3 == 0 else None)
    d["signature"] = _rand_sig(r)
    return d


def render(r, d):
    """One of the four json.dumps renderings (ensure_ascii x separator style)."""
    sep = r.choice([(",", ":"), (", ", ": ")])
    return json.dumps(d, ensure_ascii=r.choice([True, False]), separators=sep).encode("utf-8")


def _nest(depth, leaf="1"):
    return "[" * depth + leaf + "]" * depth


def edge_texts():
    """Hand-written texts, one just inside and one just outside each limit."""
    sig = _rand_sig(random.Random(5))
    head = '{"identifier":"idr","signature":"%s"' % sig

    def req(extra=""):
        return (head + extra + "}").encode()

    def padded(total):
        base = req(',"p":""')
        return req(',"p":"%s"' % ("x" * (total - len(base))))

    out = [padded(4095), padded(4096), padded(4097)]
    assert [len(t) for t in out] == [4095, 4096, 4097]
    for members in (32, 33):  # identifier + signature + the rest
        out.append(req("".join(',"k%02d":%d' % (j, j) for j in range(members - 2))))
    out += [req(',"d":' + _nest(7)), req(',"d":' + _nest(8)),  # the top-level object is level 1
            req(',"d":' + "{\"a\":" * 7 + "1" + "}" * 7), req(',"d":' + "{\"a\":" * 8 + "1" + "}" * 8)]
    out += [req(',"n":%s' % v) for v in ("9" * 18, "9" * 19, "-" + "9" * 18, "-" + "9" * 19, "-0", "01", "1e5", "1.0",
                                          "0", "-1", "NaN", "Infinity", "-Infinity", "+1", "1E5", "0x10", "--1", "-")]
    out += [req(',"a":1,"a":2'), req(',"o":{"a":1,"a":2}'), b"{}", b" {} ", req() + b"x", req() + b" \n",
            b" \t" + req(),
            req() + req(), b"\xff\xfe" + req().decode().encode("utf-16-le"), b"\xef\xbb\xbf" + req()]
    out += [req(',"s":"a\\%sb"' % e) for e in '"\\/bfnrt'] + [req(',"s":"\\u0041"'), req(',"s":"a\\x"'),
                                                            req(',"s":"a\\'),
                                                            req(',"k\\n":1'), req(',"o":{"k\\"":1}')]
    ident = '{"identifier":"idr"'
    out += [(ident + "}").encode(), (ident + ',"signature":""}').encode(), (ident + ',"signature":17}').encode(),
            (ident + ',"signature":null}').encode(), (ident + ',"signature":["%s"]}' % sig).encode(),
            (ident + ',"signature":"%s0"}' % sig[:-1]).encode(), (ident + ',"signature":"%sl"}' % sig[:-1]).encode(),
            (ident + ',"signature":"%s"}' % sig.replace(sig[3], "\\u00%02x" % ord(sig[3]), 1)).encode()]
    r = random.Random(9)
    for nbytes in (63, 64, 65):
        for _ in range(4):
            out.append((ident + ',"signature":"%s"}' % _rand_sig(r, nbytes)).encode())
    for zeros in (1, 2, 5):
        out.append((ident + ',"signature":"%s"}' % _rand_sig(r, 64, zeros)).encode())
    out += [(ident + ',"signature":"%s"}' % ("1" * k)).encode() for k in (63, 64, 65, 95, 96)]
    out += [(ident + ',"signature":"%s"}' % ("z" * k)).encode() for k in (86, 87, 88, 89, 95, 96)]
    with_sig = '{"signature":"%s"' % sig
    out += [(with_sig + "}").encode(), (with_sig + ',"identifier":""}').encode(),
            (with_sig + ',"identifier":5}').encode(), (with_sig + ',"identifier":null}').encode(),
            (with_sig + ',"identifier":"a\\nb"}').encode(), (with_sig + ',"identifier":["x"]}').encode(),
            ('{"identifier":"idr","operation":{"signature":"%s"}}' % sig).encode(),
            ('{"identifier":"idr","operation":{"signature":"%s","identifier":"in"},"signature":"%s"}'
             % (sig, sig)).encode(),
            ("[%s]" % req().decode()).encode(), json.dumps(req().decode()).encode(), b"", b" ", b"{", b"nul", b"7",
            req(',"e":[]'), req(',"e":{}'), req(',"e":[[],[]]'), req(',"e":[{},1]'), req(',"":0'), req(',"e":[1,]'),
            req(',"e":[,1]'), req(',"e":[1 2]'), req(',"e":{"a":1,}'), req(',"e":{"a" 1}'), req(',"e":tru'),
            req(',"e":truex'), req(',"e":nullnull'), req(',"e":"unterminated'), req(',"e":[1}'), req(',"e":{"a":1]'),
            req(',"t":true,"f":false,"z":null,"l":[true,false,null]'), req(',\n"w" :\t[ 1 ,\r2 ] '),
            req(',"a b":1,"a!b":2,"a":3,"a\\"":4'), req(',"ab":1,"a":2,"b":3,"aa":4,"B":5,"~":6')]
    return out


def _mutate(r, t):
    t = bytearray(t)
    for _ in range(r.randrange(1, 3)):
        if not t:
            break
        k = r.randrange(4)
        p = r.randrange(len(t))
        if k == 0:
            t[p] = r.choice(b'"\\{}[],:0123456789-.eEtfnu \t\n\x00\x7f\x80\xff') if r.randrange(2) else r.randrange(256)
        elif k == 1:
            del t[p]
        elif k == 2:
            t.insert(p, r.choice(b'"\\{}[],:01- \n'))
        else:
            t[p] ^= 1 << r.randrange(8)
    return bytes(t)


_CORPUS = []


def corpus():
    """The shared corpus (fixed seed, built once): NYM-shaped texts, renderings of request
    dicts over fuzz objects, byte mutations of both, and the edge texts."""
    if _CORPUS:
        return _CORPUS
    r = random.Random(20240611)
    base = [render(r, nym_dict(r, i)) for i in range(400)]
    for i in range(1400):
        d = {"identifier": r.choice(["L5AD5g65TDQr1PPHHRoiGf", "idr %d" % i, "x"]), "reqId": r.randrange(1 << 50),
             "operation": _rand_obj(r, 1), "signature": _rand_sig(r, 64, r.choice([0, 0, 0, 1]))}
        if r.randrange(4) == 0:
            d[r.choice(["protocolVersion", "taaAcceptance", "endorser", "zz", "A"])] = _rand_obj(r, 2)
        base.append(render(r, d))
    texts = list(base)
    texts += [_mutate(r, r.choice(base)) for _ in range(1800)]
    texts += edge_texts()
    _CORPUS.extend(texts)
    return _CORPUS


# ------------------------------------------------------------------ the CPU twin
def pack_texts(texts, base=0):
    """(uint8 buffer with `base` filler bytes in front, uint64 offsets[n + 1] starting at base)."""
    import numpy as np
    off = np.zeros(len(texts) + 1, np.uint64)
    off[0] = base
    if texts:
        off[1:] = base + np.cumsum([len(t) for t in texts])
    return np.frombuffer(b"#" * base + b"".join(texts), np.uint8), off


def twin_scan(lib, buf, off):
    """libedv_hostcheck.so hc_wire_scan over packed texts: (status[n], idr_span[n, 2],
    sig64[n, 64], msgs (item i at off[i] - off[0]), msg_len[n])."""
    import ctypes

    import numpy as np
    n = len(off) - 1
    buf = np.ascontiguousarray(buf, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    status = np.zeros(n, np.uint8)
    span = np.zeros((n, 2), np.uint32)
    sig = np.zeros((n, 64), np.uint8)
    msgs = np.zeros(max(1, int(off[-1] - off[0])), np.uint8)
    mlen = np.zeros(n, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.hc_wire_scan.restype = None
    lib.hc_wire_scan(P(buf), P(off), ctypes.c_uint64(n), P(status), P(span), P(sig), P(msgs), P(mlen))
    return status, span, sig, msgs, mlen
