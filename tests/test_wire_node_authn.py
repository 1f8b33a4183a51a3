"""authenticate_node_wire_batch on the host: per entry, what authenticate_batch returns for
batching.requests_in_drain of the same entries, over unwrapped, host-decided and empty
messages alike.  The engine is wire_node_double's WireNodeOracleEngine (the kernels' lane
code on the CPU, the C oracle's verdicts)."""
import json
import random

import pytest

import wire_model
import wire_unwrap_model as wum
from engine_double import OracleEngine
from plenum_amd.batching import requests_in_drain
from plenum_amd.client_authn import GpuAuthNr, ReqAuthenticator
from plenum_amd.nodeloop import batch_text, propagate_text
from test_wire_authn import _Raising, _Signer, _register, _same
from wire_idents_double import WireIdentsOracleEngine
from wire_node_double import WireNodeOracleEngine


@pytest.fixture(scope="module")
def drain(oracle):
    """A mixed node drain: client requests, bare PROPAGATEs and BATCHes of signed NYM requests
    (every third S corrupted; signers known, unknown, with a None verkey, or whose getVerkey
    raises), PREPARE-like members, and the unwrap corpus (declined BATCHes, nested ones, \\u
    escapes, undecodable entries, truncations)."""
    r = random.Random(12)
    signers = [_Signer(oracle, k) for k in range(8)]
    reqs = []
    for i in range(240):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        if i % 13 == 0:
            d["operation"]["amount"] = 1.5  # the scan leaves it to the host (a float), which verifies
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        reqs.append(d)
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(reqs)]
    prepare = json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 3, "digest": "d", "txnRootHash": None})
    entries = [json.dumps(d) for d in reqs[:40]] + props[40:80]
    for k in range(80, 240, 40):
        entries.append(batch_text(props[k:k + 20] + [prepare] + props[k + 20:k + 40] + [prepare]))
    entries.append(batch_text([]))
    entries.append(batch_text([props[0].replace("client0", "client\\u0030"), props[1], prepare]))
    entries.append(batch_text([batch_text(props[2:5]), props[5]]))
    entries = [e.encode() for e in entries]
    corp = wum.corpus()
    entries += corp["clean"] + corp["mutated"]
    r.shuffle(entries)
    return signers, entries


def _host_definition(a, entries):
    return a.authenticate_batch(requests_in_drain(entries))


def _assert_same(entries, got, want):
    assert len(got) == len(entries)
    assert [len(g) for g in got] == [len(requests_in_drain([e])) for e in entries]
    flat = [x for g in got for x in g]
    assert len(flat) == len(want)
    for i, (g, w) in enumerate(zip(flat, want)):
        assert _same(g, w), (i, g, w)


def test_node_wire_batch_equals_the_host_definition(oracle, hostcheck, drain):
    signers, entries = drain
    wire = _register(_Raising(engine=WireNodeOracleEngine(oracle, hostcheck)), signers)
    plain = _register(_Raising(engine=OracleEngine(oracle)), signers)
    got = wire.authenticate_node_wire_batch(entries)
    want = _host_definition(plain, entries)
    _assert_same(entries, got, want)
    kinds = {type(w).__name__ for w in want}
    assert {"str", "InvalidSignature", "UnknownIdentifier", "CouldNotAuthenticate"} <= kinds, kinds
    assert sum(isinstance(w, str) for w in want) >= 60  # (5 signers of 8 verify, 2 signatures of 3 are intact)
    # what went where: the messages the model classes, against the counters
    cls = [wum.unwrap(b, e)[0] for b, e in wum.messages(entries)]
    st = wire.stats
    assert st["wire_items"] + st["wire_host_items"] == len(cls) - cls.count(wum.NONE)
    assert st["wire_host_items"] >= cls.count(wum.HOST) >= 50  # (+ the requests the scan left to the host)
    assert st["wire_items"] >= 300
    eng = wire.engine
    assert (eng.node_scans, eng.wire_idents_calls, eng.ident_text_calls, eng.wire_verifies) == (1, 1, 1, 1)
    assert wire._g.last_wire_breakdown["items"] == len(cls)


def test_getverkey_once_per_distinct_gpu_handled_identifier(oracle, hostcheck, drain):
    signers, entries = drain
    clean = [e for e in entries if e in set(wum.corpus()["clean"])] + [e for e in entries if b"client1" in e][:8]
    a = _register(_Raising(engine=WireNodeOracleEngine(oracle, hostcheck)), signers)
    a.authenticate_node_wire_batch(clean)
    seen = []
    for body, esc in wum.messages(clean):
        cls, out = wum.unwrap(body, esc)
        if cls == wum.REQUEST and wire_model.scan(out) is not None:
            sig = wire_model.scan(out)[2]
            if len(sig) in range(86, 90):
                seen.append(wire_model.scan(out)[1])
    # (a signature text of that length may still not decode to 64 bytes: the twin decides)
    assert set(a.seen) <= set(seen) and len(a.seen) == len(set(a.seen)) and len(a.seen) >= 20
    assert a.seen == [s for s in dict.fromkeys(seen) if s in set(a.seen)]  # first-occurrence order


def test_steady_drain_is_one_keyed_verify(oracle, hostcheck):
    """Only PROPAGATEs in BATCHes, every key registered: no host message, every item keyed."""
    r = random.Random(6)
    signers = [_Signer(oracle, k) for k in range(4)]
    reqs = []
    for i in range(140):
        d = wire_model.nym_dict(r, i)
        d["identifier"] = signers[i % 4].idr
        sig = bytearray(signers[i % 4].sign(d))
        if i % 5 == 0:
            sig[3] ^= 2
        d["signature"] = wire_model.b58(bytes(sig))
        reqs.append(d)
    props = [propagate_text(d, "c%d" % i) for i, d in enumerate(reqs)]
    entries = [batch_text(props[:70]).encode(), batch_text(props[70:]).encode()]
    wire, plain = (GpuAuthNr(engine=e) for e in (WireNodeOracleEngine(oracle, hostcheck), OracleEngine(oracle)))
    for a in (wire, plain):
        for s in signers:
            a.addIdr(s.idr, s.abbreviated)
        a.keys_settle()
    got = wire.authenticate_node_wire_batch(entries)
    _assert_same(entries, got, _host_definition(plain, entries))
    assert [len(g) for g in got] == [70, 70]
    assert [isinstance(x, str) for g in got for x in g] == [i % 5 != 0 for i in range(140)]
    st = wire.stats
    assert st["wire_items"] == st["keyed_items"] == st["batch_items"] == 140 and st["wire_host_items"] == 0
    assert wire.engine.wire_verify_idents_calls == 1 and wire.engine.wire_verifies == 0


@pytest.mark.parametrize("engine", [OracleEngine, WireIdentsOracleEngine])
def test_engine_without_the_node_path_takes_the_host_definition(oracle, hostcheck, drain, engine):
    signers, entries = drain
    entries = entries[:150]
    make = (lambda: engine(oracle)) if engine is OracleEngine else (lambda: engine(oracle, hostcheck))
    a = _register(_Raising(engine=make()), signers)
    b = _register(_Raising(engine=OracleEngine(oracle)), signers)
    _assert_same(entries, a.authenticate_node_wire_batch(entries), _host_definition(b, entries))
    assert a.stats["wire_items"] == 0 and a.stats["wire_host_items"] == len(entries)
    assert getattr(a.engine, "wire_scans", 0) == 0


def test_other_inputs_and_the_aggregator(oracle, hostcheck, drain):
    signers, entries = drain
    few = entries[:60]
    a = _register(GpuAuthNr(engine=WireNodeOracleEngine(oracle, hostcheck)), signers)
    assert a.authenticate_node_wire_batch([]) == []
    assert a.authenticate_node_wire_batch([batch_text([]).encode()] * 3) == [[], [], []]
    want = _host_definition(_register(GpuAuthNr(engine=OracleEngine(oracle)), signers), few)
    _assert_same(few, a.authenticate_node_wire_batch(tuple(few)), want)  # not a list: the host definition
    as_str = [t.decode("latin-1") if i % 2 else t for i, t in enumerate(few)]  # not all bytes
    _assert_same(as_str, a.authenticate_node_wire_batch(as_str),
                 _host_definition(_register(GpuAuthNr(engine=OracleEngine(oracle)), signers), as_str))
    ra = ReqAuthenticator()
    ra.register_authenticator(a)
    _assert_same(few, ra.authenticate_node_wire_batch(few), want)
