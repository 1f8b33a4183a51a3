"""authenticate_node_wire_batch with the BATCHes split by the device code (wire_split_double's
WireSplitOracleEngine: hc_node_split_lanes, then the existing twins) against the same call with
the host split and against the host definition, authenticate_batch over
batching.requests_in_drain: the same results, the same counters, getVerkey called alike."""
import json
import random

import pytest

import wire_model
import wire_unwrap_model as wum
from engine_double import OracleEngine
from plenum_amd.batching import requests_in_drain
from plenum_amd.client_authn import GpuAuthNr
from plenum_amd.nodeloop import batch_text, propagate_text
from test_wire_authn import _Raising, _Signer, _register, _same
from wire_node_double import WireNodeOracleEngine
from wire_split_double import WireSplitOracleEngine


@pytest.fixture(scope="module")
def drain(oracle):
    """3 client requests, 2 bare PROPAGATEs, 3 BATCHes of 70 members (signed NYM requests, every
    third S corrupted; signers known, unknown, with a None verkey, or whose getVerkey raises;
    PREPARE-like members), one member with a \\u escape (the host decodes it), a nested BATCH, an
    empty one, an undecodable entry -- and the unwrap corpus."""
    r = random.Random(77)
    signers = [_Signer(oracle, k) for k in range(8)]
    reqs = []
    for i in range(3 + 2 + 3 * 68):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        reqs.append(d)
    prepare = json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 9, "digest": "d", "txnRootHash": None})
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(reqs)]
    props[50] = props[50].replace("client50", "client\\u0035\\u0030")  # the same message, host-decoded
    entries = [json.dumps(d) for d in reqs[:3]] + props[3:5]
    for b in range(3):
        members = props[5 + 68 * b:5 + 68 * (b + 1)]
        entries.append(batch_text(members[:30] + [prepare] + members[30:] + [prepare]))
    entries.insert(4, '{"op": "PROPAGATE", "request": {"signature": ')  # undecodable
    entries.append(batch_text([]))
    entries.append(batch_text([batch_text(props[6:9]), props[9]]))
    drain_entries = [e.encode() for e in entries]
    corp = wum.corpus()
    return signers, drain_entries, corp["clean"] + corp["mutated"]


def _pair(oracle, hostcheck, signers, cls=_Raising):
    gpu, host = (_register(cls(engine=WireSplitOracleEngine(oracle, hostcheck)), signers) for _ in range(2))
    gpu._g.wire_split_gpu = True
    host._g.wire_split_gpu = False
    return gpu, host


def _assert_both_paths(oracle, hostcheck, signers, entries):
    gpu, host = _pair(oracle, hostcheck, signers)
    plain = _register(_Raising(engine=OracleEngine(oracle)), signers)
    got = gpu.authenticate_node_wire_batch(entries)
    other = host.authenticate_node_wire_batch(entries)
    want = plain.authenticate_batch(requests_in_drain(entries))
    assert gpu.engine.entry_scans == 1 and gpu.engine.node_scans == 0
    assert host.engine.entry_scans == 0 and host.engine.node_scans == 1
    assert [len(g) for g in got] == [len(g) for g in other] == [len(requests_in_drain([e])) for e in entries]
    flat, flat_other = [x for g in got for x in g], [x for g in other for x in g]
    assert len(flat) == len(flat_other) == len(want)
    for i, (g, o, w) in enumerate(zip(flat, flat_other, want)):
        assert _same(g, o) and _same(g, w), (i, g, o, w)
    assert gpu.stats == host.stats
    # getVerkey: the same calls in the same order (once per distinct identifier of the GPU-handled
    # items, first occurrence first; then authenticate_batch's own for the host-decoded ones)
    assert gpu.seen == host.seen and len(gpu.seen) >= 8
    assert set(gpu._g.last_wire_breakdown) == set(host._g.last_wire_breakdown)
    assert gpu._g.last_wire_breakdown["items"] == host._g.last_wire_breakdown["items"]
    assert gpu._g.last_wire_breakdown["host_items"] == host._g.last_wire_breakdown["host_items"]
    return gpu, want


def test_the_drain_on_both_paths(oracle, hostcheck, drain):
    signers, entries, _ = drain
    gpu, want = _assert_both_paths(oracle, hostcheck, signers, entries)
    kinds = {type(w).__name__ for w in want}
    assert {"str", "InvalidSignature", "UnknownIdentifier", "CouldNotAuthenticate"} <= kinds, kinds
    cls = [wum.unwrap(b, e)[0] for b, e in wum.messages(entries)]
    assert cls.count(wum.HOST) >= 3  # the \u member, the nested BATCH, the undecodable entry
    assert gpu.stats["wire_host_items"] >= cls.count(wum.HOST) and gpu.stats["wire_items"] >= 200


def test_the_corpus_on_both_paths(oracle, hostcheck, drain):
    signers, entries, corpus = drain
    mixed = corpus + entries
    random.Random(5).shuffle(mixed)
    _assert_both_paths(oracle, hostcheck, signers, mixed)


def test_fallbacks_are_the_same_on_both_paths(oracle, hostcheck, drain):
    signers, entries, _ = drain
    gpu, host = _pair(oracle, hostcheck, signers, GpuAuthNr)
    plain = _register(GpuAuthNr(engine=OracleEngine(oracle)), signers)
    for a in (gpu, host):
        assert a.authenticate_node_wire_batch([]) == []
        assert a.authenticate_node_wire_batch([batch_text([]).encode()] * 3) == [[], [], []]
    assert gpu.engine.entry_scans == 1 and gpu.engine.wire is None  # (no message: nothing scanned)
    few = entries[:9]
    as_str = [t.decode("latin-1") if i % 2 else t for i, t in enumerate(few)]  # not all bytes
    for arg in (tuple(few), as_str):
        want = plain.authenticate_batch(requests_in_drain(list(arg)))
        for a in (gpu, host):
            flat = [x for g in a.authenticate_node_wire_batch(arg) for x in g]
            assert len(flat) == len(want) and all(_same(g, w) for g, w in zip(flat, want))
    assert gpu.stats == host.stats and gpu.engine.entry_scans == 1
    # a short buffer estimate: the second gather takes the entries' own size
    for a in (gpu, host):
        a._g.node_wire_bytes_per_entry = 1.0
        a._g.__dict__.pop("wire_text_plain", None)
    want = plain.authenticate_batch(requests_in_drain(entries))
    for a in (gpu, host):
        flat = [x for g in a.authenticate_node_wire_batch(entries) for x in g]
        assert len(flat) == len(want) and all(_same(g, w) for g, w in zip(flat, want))
    assert gpu.stats == host.stats and gpu.engine.entry_scans == 2


def test_an_engine_without_the_split_takes_the_host_split(oracle, hostcheck, drain):
    signers, entries, _ = drain
    a = _register(_Raising(engine=WireNodeOracleEngine(oracle, hostcheck)), signers)
    assert a._g.wire_split_gpu in (True, False) and not getattr(a.engine, "supports_wire_split", False)
    a._g.wire_split_gpu = True
    got = a.authenticate_node_wire_batch(entries)
    want = _register(_Raising(engine=OracleEngine(oracle)), signers).authenticate_batch(requests_in_drain(entries))
    flat = [x for g in got for x in g]
    assert len(flat) == len(want) and all(_same(g, w) for g, w in zip(flat, want))
    assert a.engine.node_scans == 1
