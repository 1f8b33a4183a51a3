"""The node-message unwrap and the BATCH splitter on the CPU: the Python restatement
(wire_unwrap_model) against batching.requests_in_drain and json.loads, and the C++ twin
(libedv_hostcheck.so hc_wire_unwrap, every access asserted in bounds) and
_hostpack.gather_node_texts against the restatement, byte for byte."""
import json

import numpy as np
import pytest

import wire_model
import wire_unwrap_model as wum
from plenum_amd import _hostpack
from plenum_amd.batching import requests_in_drain


@pytest.fixture(scope="module")
def corp():
    return wum.corpus()


def _as_entry(body, esc):
    """What requests_in_drain sees of a message: the entry itself, or the BATCH member the body
    was cut from (a str inside a BATCH dict, so that it is visited one level down as in the
    entry it came from); None where the body is no JSON string body, which the splitter never
    cuts out."""
    if not esc:
        return body
    try:
        return {"op": "BATCH", "messages": [json.loads(b'"' + body + b'"')]}
    except ValueError:
        return None


def _check_message(body, esc):
    cls, out = wum.unwrap(body, esc)
    assert len(out) == len(body) and cls in (wum.REQUEST, wum.HOST, wum.NONE)
    entry = _as_entry(body, esc)
    assert entry is not None, body  # (the splitter only cuts out well-formed string bodies)
    got = requests_in_drain([entry])
    if cls == wum.NONE:
        assert got == [], body
        assert out == b" " * len(body)
    elif cls == wum.REQUEST:
        # The unwrap validates the envelope, the scan validates the request object (a whole
        # object that is the request is not parsed twice): so the claim is made of the request
        # text as json.loads sees it.  Text json.loads rejects must be text the scanner leaves to
        # the host, and then the message holds nothing.
        try:
            d = json.loads(out)
        except ValueError:
            assert wire_model.scan(out) is None and got == [], body
        else:
            assert got == [d], body
    else:
        assert out == b" " * len(body)
    return cls


def test_every_message_against_requests_in_drain(corp):
    seen = {wum.REQUEST: 0, wum.HOST: 0, wum.NONE: 0}
    for family in ("clean", "mutated"):
        for body, esc in wum.messages(corp[family]):
            seen[_check_message(body, esc)] += 1
    # every entry whole as well, as the GPU meets an entry the splitter declines
    for raw in corp["clean"] + corp["mutated"]:
        seen[_check_message(raw, 0)] += 1
    assert min(seen.values()) >= 40, seen


def test_split_bodies_are_the_strings_json_loads_holds(corp):
    split = 0
    for raw in corp["clean"] + corp["mutated"]:
        bodies = wum.split(raw)
        if bodies is None:
            continue
        split += 1
        d = json.loads(raw)  # an entry the model splits is one json.loads accepts
        assert d["op"] == "BATCH"
        assert [json.loads(b'"' + b + b'"') for b in bodies] == d["messages"]
    assert split >= 10


def test_the_unmutated_family_stays_on_the_gpu(corp):
    """Straight json.dumps output over ASCII requests: no message the host decides, no BATCH
    left unsplit (so the tests above cannot pass by sending everything to the host)."""
    batches = 0
    for raw in corp["clean"]:
        is_batch = json.loads(raw).get("op") == "BATCH"
        batches += is_batch
        assert (wum.split(raw) is not None) == is_batch, raw
    assert batches >= 5
    requests = 0
    for body, esc in wum.messages(corp["clean"]):
        cls, out = wum.unwrap(body, esc)
        assert cls != wum.HOST, body
        if cls == wum.REQUEST:
            requests += 1
            assert wire_model.scan(out) is not None, body  # and the scanner takes the request
    assert requests >= 90
    assert {len(wum.split(raw)) for raw in corp["clean"] if wum.split(raw) is not None} >= {0, 1, 2, 70}


def test_the_limits(corp):
    by_len = {len(t): t for t in corp["mutated"] if len(t) in (4095, 4096, 4097)}
    assert [wum.unwrap(by_len[k], 0)[0] for k in (4095, 4096, 4097)] == [wum.REQUEST, wum.REQUEST, wum.HOST]
    members = [t for t in corp["mutated"] if t.count(b'"k0') >= 10]
    assert sorted(wum.unwrap(t, 0)[0] for t in members) == [wum.REQUEST, wum.REQUEST, wum.HOST, wum.HOST]


def _packed(entries):
    buf, off, esc, entry = wum.gather(entries)
    return (np.frombuffer(buf, np.uint8), np.array(off, np.uint64), np.array(esc, np.uint8),
            np.array(entry, np.uint32))


def test_twin_equals_the_model(corp, hostcheck):
    entries = corp["clean"] + corp["mutated"]
    for group in (entries, [e for e in entries if wum.split(e) is None]):
        buf, off, esc, _ = _packed(group)
        cls, out = wum.twin_unwrap(hostcheck, buf, off, esc)
        want = [wum.unwrap(buf[int(a):int(b)].tobytes(), int(e)) for a, b, e in zip(off[:-1], off[1:], esc)]
        assert cls.tolist() == [c for c, _ in want]
        assert out.tobytes() == b"".join(o for _, o in want)
    # every entry whole too (esc = 0 for a BATCH the splitter would have cut)
    buf, off = wire_model.pack_texts(entries)
    cls, out = wum.twin_unwrap(hostcheck, buf, off, np.zeros(len(entries), np.uint8))
    want = [wum.unwrap(e, 0) for e in entries]
    assert cls.tolist() == [c for c, _ in want] and out.tobytes() == b"".join(o for _, o in want)
    # ... and every message as an escaped body, whatever it is: the unescape's own refusals
    cls, out = wum.twin_unwrap(hostcheck, buf, off, np.ones(len(entries), np.uint8))
    want = [wum.unwrap(e, 1) for e in entries]
    assert cls.tolist() == [c for c, _ in want] and out.tobytes() == b"".join(o for _, o in want)


@pytest.mark.parametrize("threads", [1, 4])
def test_gather_node_texts_equals_the_model(corp, threads):
    entries = (corp["clean"] + corp["mutated"]) * 3  # more than one chunk of entries
    buf, off, esc, entry = _packed(entries)
    out = bytearray(len(buf) + 64)
    got = _hostpack.gather_node_texts(entries, out, threads)
    assert got is not None
    g_off, g_esc, g_entry = (np.frombuffer(b, t) for b, t in zip(got, (np.uint64, np.uint8, np.uint32)))
    assert g_off.tolist() == off.tolist()
    assert g_esc.tolist() == esc.tolist()
    assert g_entry.tolist() == entry.tolist()
    assert bytes(out[:len(buf)]) == buf.tobytes()
    assert (np.diff(g_entry.astype(np.int64)) >= 0).all()


def test_gather_node_texts_refuses_what_it_cannot_take(corp):
    entries = corp["clean"][:30]
    need = len(wum.gather(entries)[0])
    assert _hostpack.gather_node_texts(entries, bytearray(need - 1)) is None
    assert _hostpack.gather_node_texts(entries, bytearray(need)) is not None
    assert _hostpack.gather_node_texts(entries + ["text"], bytearray(need + 64)) is None
    assert _hostpack.gather_node_texts(tuple(entries), bytearray(need)) is None
    off, esc, entry = _hostpack.gather_node_texts([], bytearray(8))
    assert (len(off), len(esc), len(entry)) == (8, 0, 0)
