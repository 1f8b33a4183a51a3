"""The entries the device BATCH split is held to the host's on (csrc/node_split_lanes.h against
csrc/node_split.h), shared by the CPU and GPU tests: the node corpus, a boundary sweep over the
lane edges and the wave's steps, and member counts around the wave's width.  Also the CPU twin's
binding (libedv_hostcheck.so hc_node_split_lanes) and the host's answer in the same shape."""
import ctypes

import numpy as np

import wire_unwrap_model as wum

_HEAD = b'{"op":"BATCH","messages":['
_TAIL = b'],"signature":null}'
_CACHE = {}


def batch_of(bodies, head=_HEAD, tail=_TAIL):
    """A BATCH whose member strings have exactly these (already escaped) bodies."""
    return head + b",".join(b'"' + b + b'"' for b in bodies) + tail


def corpus_entries():
    c = wum.corpus()
    return c["clean"] + c["mutated"]


def sweep_entries():
    """One-member BATCHes whose body is x*p + backslash*r + quote + y: the backslash run and the
    quote after it end at every offset across the 16-byte lane edges and the first two 1,024-byte
    steps (the kernel's steps start at the 16-byte boundary at or before the entry, so p also runs
    over 1990..2029: the second step's edge for every alignment of the entry).  An odd r continues
    the member (split), an even r ends it and leaves a stray y (not split)."""
    if "sweep" not in _CACHE:
        out = []
        for r in (1, 2, 3, 4):
            for p in list(range(0, 1100)) + list(range(1990, 2070)):
                out.append(batch_of([b"x" * p + b"\\" * r + b'"' + b"y"]))
        _CACHE["sweep"] = out
    return _CACHE["sweep"]


def count_entries():
    """0, 1, 2, 63, 64, 65, 70 and 130 members with empty ones among them, empty BATCHes between
    split ones, whitespace around every token, and entries of exactly 1,023, 1,024 and 1,025 bytes."""
    if "count" not in _CACHE:
        out = []
        for k in (0, 1, 2, 63, 64, 65, 70, 130):
            bodies = [b"" if j % 7 == 3 else b'{\\"n\\":%d,\\"s\\":\\"a\\\\\\\\b\\/c\\"}' % j for j in range(k)]
            out.append(batch_of(bodies))
            out.append(batch_of([]))
            out.append(batch_of(bodies, head=b' { "op" : "BATCH" , "messages" : [ ', tail=b' ] , "signature" : null } '))
        out.append(batch_of([b""]))
        out.append(batch_of([b"", b"", b""]))
        out.append(b'{"op":"BATCH","messages":[  ]}')
        out.append(batch_of([b"a"] * 40, tail=b' ],"n":-12,"t":true,"f":false,"s":"x y","z":0}  '))
        out.append(batch_of([b"a"] * 40, tail=b'],"n":-0}'))
        out.append(batch_of([b"a", b"b"]).replace(b'","', b'" "'))
        out.append(batch_of([b"a", b"b"])[:-1])
        for total in (1023, 1024, 1025):
            short = batch_of([b"m" * 10, b""])
            out.append(batch_of([b"m" * (10 + total - len(short)), b""]))
            assert len(out[-1]) == total
            out.append(batch_of([b"m" * (10 + total - len(short) - 1) + b"\\", b""]))  # (the quote escaped)
            out.append((b'{"op":"PROPAGATE","k":"' + b"z" * total)[:total - 2] + b'"}')
            assert len(out[-1]) == total
        _CACHE["count"] = out
    return _CACHE["count"]


def pack(entries, base=0):
    """(text uint8[base + bytes], entry_off uint64[n + 1] from base)."""
    off = np.zeros(len(entries) + 1, np.uint64)
    np.cumsum([len(e) for e in entries], out=off[1:])
    off += np.uint64(base)
    return np.frombuffer(b"\0" * base + b"".join(entries), np.uint8), off


def host_split(entries):
    """_hostpack.gather_node_texts: (off uint64[m + 1], esc uint8[m], entry uint32[m], bodies uint8)."""
    from plenum_amd import _hostpack
    out = bytearray(sum(map(len, entries)) + 1)
    got = _hostpack.gather_node_texts(list(entries), out)
    assert got is not None
    off = np.frombuffer(got[0], np.uint64)
    return off, np.frombuffer(got[1], np.uint8), np.frombuffer(got[2], np.uint32), \
        np.frombuffer(bytes(out[:int(off[-1])]), np.uint8)


def twin_split(lib, text, entry_off):
    """libedv_hostcheck.so hc_node_split_lanes: (off, esc, entry, at) as the device passes make them."""
    text = np.ascontiguousarray(text, np.uint8)
    entry_off = np.ascontiguousarray(entry_off, np.uint64)
    n_e = len(entry_off) - 1
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = lib.hc_node_split_lanes
    fn.restype = ctypes.c_int64
    nb = ctypes.c_uint64(0)
    m = fn(P(text), P(entry_off), ctypes.c_uint64(n_e), ctypes.c_uint64(0), None, None, None, None, ctypes.byref(nb))
    off = np.zeros(m + 1, np.uint64)
    esc = np.zeros(m, np.uint8)
    entry = np.zeros(m, np.uint32)
    at = np.zeros(m, np.uint64)
    again = fn(P(text), P(entry_off), ctypes.c_uint64(n_e), ctypes.c_uint64(m), P(off), P(esc), P(entry), P(at),
               ctypes.byref(nb))
    assert again == m and int(off[-1]) == nb.value
    return off, esc, entry, at


def bodies_at(text, off, at):
    """The messages' bytes taken from the entries at `at`, back to back."""
    text = np.ascontiguousarray(text, np.uint8)
    lens = np.diff(off).astype(np.int64)
    if len(lens) == 0:
        return np.zeros(0, np.uint8)
    idx = np.repeat(at.astype(np.int64) - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]), dtype=np.int64)
    return text[idx]
