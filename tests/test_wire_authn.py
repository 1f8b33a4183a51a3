"""authenticate_wire_batch on the host: element-wise what authenticate_batch returns for the
decoded texts, over scanned and host-decided items alike.  The engine is wire_double's
WireOracleEngine (the kernel's lane code on the CPU, the C oracle's verdicts)."""
import ctypes
import json
import random

import pytest

import wire_model
from engine_double import OracleEngine
from plenum_amd.client_authn import GpuAuthNr, ReqAuthenticator
from wire_double import WireOracleEngine


def _same(a, b):
    if isinstance(b, Exception):
        return (type(a) is type(b) and a.args == b.args and type(a.__cause__) is type(b.__cause__)
                and getattr(a.__cause__, "args", None) == getattr(b.__cause__, "args", None))
    return a == b and type(a) is type(b)


class _Signer:
    def __init__(self, oracle, k):
        self.oracle = oracle
        self.pk, self.sk = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        oracle.oracle_seed_keypair(self.pk, self.sk, bytes([7, k + 1]) + b"\0" * 30)
        self.idr = wire_model.b58(self.pk.raw[:16])
        self.abbreviated = "~" + wire_model.b58(self.pk.raw[16:])
        self.full = wire_model.b58(self.pk.raw)

    def sign(self, d):
        from plenum_amd.serialization import serialize_msg_for_signing
        ser = serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"])
        sig = ctypes.create_string_buffer(64)
        self.oracle.oracle_sign_detached(sig, ser, ctypes.c_uint64(len(ser)), self.sk)
        return sig.raw


class _Raising(GpuAuthNr):
    """getVerkey raises for some identifiers and counts its calls."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def getVerkey(self, identifier):
        self.seen.append(identifier)
        if identifier.startswith("boom"):
            raise KeyError(identifier)
        return super().getVerkey(identifier)


@pytest.fixture(scope="module")
def signed_slice(oracle):
    """About 3,000 texts: signed NYM requests (every third S corrupted) from signers known by an
    abbreviated verkey, by a full one under another identifier, with a None verkey, unknown, or
    whose getVerkey raises; corpus texts (fuzz renderings, mutations, the edge texts -- scanned
    ones with unverifiable signatures, host-decided ones, unparsable ones)."""
    r = random.Random(4)
    signers = [_Signer(oracle, k) for k in range(8)]
    texts = []
    for i in range(360):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        if i % 11 == 0:
            d["operation"]["amount"] = 1.5  # the host decides (a float), and verifies
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        texts.append(wire_model.render(r, d))
    corpus = wire_model.corpus()
    texts += corpus[400:400 + 1500] + corpus[-1200:]
    r.shuffle(texts)
    return signers, texts


def _register(a, signers):
    for k, s in enumerate(signers):
        if k < 4:
            a.addIdr(s.idr, s.abbreviated)
        elif k == 4:
            a.addIdr(s.idr, None)
        elif k == 5:
            a.addIdr("full-key-5", s.full)
    a.addIdr("idr", "~short")  # the edge texts' identifier: a verkey DidVerifier cannot use
    return a


def _decoded_results(a, texts):
    """authenticate_batch over the decoded texts, the decoder's exception where it raises."""
    want, idx, decoded = [None] * len(texts), [], []
    for i, t in enumerate(texts):
        try:
            decoded.append(json.loads(t))
            idx.append(i)
        except ValueError as ex:
            want[i] = ex
    for i, res in zip(idx, a.authenticate_batch(decoded)):
        want[i] = res
    return want


def test_wire_batch_equals_dict_batch(oracle, hostcheck, signed_slice):
    signers, texts = signed_slice
    wire = _register(_Raising(engine=WireOracleEngine(oracle, hostcheck)), signers)
    plain = _register(_Raising(engine=OracleEngine(oracle)), signers)
    got = wire.authenticate_wire_batch(texts)
    want = _decoded_results(plain, texts)
    assert len(got) == len(want) == len(texts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (i, texts[i], g, w)
    kinds = {type(w).__name__ for w in want}
    assert {"str", "InvalidSignature", "UnknownIdentifier", "CouldNotAuthenticate", "JSONDecodeError",
            "UnicodeDecodeError", "MissingSignature", "InvalidSignatureFormat"} <= kinds, kinds
    assert sum(isinstance(w, str) for w in want) >= 100
    st = wire.stats
    assert st["wire_items"] + st["wire_host_items"] == len(texts)
    assert st["wire_items"] >= 1000 and st["wire_host_items"] >= 500
    assert wire.engine.wire_scans == 1 and wire.engine.wire_verifies == 1


def test_getverkey_once_per_distinct_scanned_identifier(oracle, hostcheck, signed_slice):
    signers, texts = signed_slice
    scanned = [t for t in texts if wire_model.scan(t) is not None
               and len(wire_model.scan(t)[2]) in range(86, 90) and wire_model.scan(t)[1] != "idr"]
    status = wire_model.twin_scan(hostcheck, *wire_model.pack_texts(scanned))[0]
    scanned = [t for t, s in zip(scanned, status) if s == 0]
    assert len(scanned) >= 1000
    a = _register(_Raising(engine=WireOracleEngine(oracle, hostcheck)), signers)
    a.authenticate_wire_batch(scanned)
    first_seen = list(dict.fromkeys(wire_model.scan(t)[1] for t in scanned))
    assert a.seen == first_seen  # once each, in first-occurrence order
    assert a.stats["wire_host_items"] == 0 and a.stats["wire_items"] == len(scanned)


def test_steady_state_batch_every_item_scanned_and_keyed(oracle, hostcheck):
    """Every text scanned, every signer's key registered: one keyed verify, no host item."""
    r = random.Random(6)
    signers = [_Signer(oracle, k) for k in range(4)]
    texts = []
    for i in range(200):
        d = wire_model.nym_dict(r, i)
        d["identifier"] = signers[i % 4].idr
        sig = bytearray(signers[i % 4].sign(d))
        if i % 5 == 0:
            sig[3] ^= 2
        d["signature"] = wire_model.b58(bytes(sig))
        texts.append(wire_model.render(r, d))
    wire, plain = (GpuAuthNr(engine=e) for e in (WireOracleEngine(oracle, hostcheck), OracleEngine(oracle)))
    for a in (wire, plain):
        for s in signers:
            a.addIdr(s.idr, s.abbreviated)
        a.keys_settle()
    got = wire.authenticate_wire_batch(texts)
    want = plain.authenticate_batch([json.loads(t) for t in texts])
    assert all(_same(g, w) for g, w in zip(got, want))
    assert [isinstance(g, str) for g in got] == [i % 5 != 0 for i in range(200)]
    st = wire.stats
    assert st["wire_items"] == st["keyed_items"] == st["batch_items"] == 200 and st["wire_host_items"] == 0
    assert wire.engine.keyed_calls == 1 and wire.engine.wire_verifies == 1


def test_engine_without_wire_takes_the_dict_path(oracle, signed_slice):
    signers, texts = signed_slice
    texts = texts[:600]
    a = _register(_Raising(engine=OracleEngine(oracle)), signers)
    b = _register(_Raising(engine=OracleEngine(oracle)), signers)
    got = a.authenticate_wire_batch(texts)
    for i, (g, w) in enumerate(zip(got, _decoded_results(b, texts))):
        assert _same(g, w), (i, texts[i], g, w)
    assert a.stats["wire_items"] == 0 and a.stats["wire_host_items"] == len(texts)


def test_other_inputs_and_the_aggregator(oracle, hostcheck, signed_slice):
    signers, texts = signed_slice
    a = _register(GpuAuthNr(engine=WireOracleEngine(oracle, hostcheck)), signers)
    assert a.authenticate_wire_batch([]) == []
    few = texts[:50]
    want = _decoded_results(_register(GpuAuthNr(engine=OracleEngine(oracle)), signers), few)
    as_str = [t.decode("latin-1") if i % 2 else t for i, t in enumerate(few)]  # not all bytes: decoded on the host
    want_str = []
    for t in as_str:
        try:
            want_str.append(json.loads(t))
        except ValueError as ex:
            want_str.append(ex)
    got = a.authenticate_wire_batch(tuple(few))
    assert all(_same(g, w) for g, w in zip(got, want))
    ra = ReqAuthenticator()
    ra.register_authenticator(a)
    assert all(_same(g, w) for g, w in zip(ra.authenticate_wire_batch(few), want))
    got = a.authenticate_wire_batch(as_str)
    assert [isinstance(g, ValueError) for g in got] == [isinstance(w, ValueError) for w in want_str]
