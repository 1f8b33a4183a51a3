"""authenticate_node_wire_batch with the work-list verify (wire_list_double's
WireListOracleEngine: hc_wire_once for the representatives, the C oracle's verdicts over them)
against the host definition, for the list on / off x once on / off: the same results, the same
counters, and with the list on not one per-item wire_verify."""
import random

import pytest

import wire_model
import wire_unwrap_model as wum
from engine_double import OracleEngine
from test_wire_authn import _Raising, _Signer, _register, _same
from wire_list_double import WireListOracleEngine, mixed_drain
from wire_split_double import WireSplitOracleEngine

EXISTING = ("batches", "batch_items", "keyed_items", "wire_items", "wire_host_items")
SETTINGS = [(False, False), (True, False), (False, True), (True, True)]  # (list, once)


@pytest.fixture(scope="module")
def drain(oracle):
    """The mixed drain over 213 signed NYM requests (every third S corrupted; signers known,
    with an unusable or a None verkey, unknown, or whose getVerkey raises), and the unwrap
    corpus."""
    r = random.Random(78)
    signers = [_Signer(oracle, k) for k in range(8)]
    reqs = []
    for i in range(3 + 3 * 70):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        reqs.append(d)
    corp = wum.corpus()
    return signers, reqs, mixed_drain(reqs), corp["clean"] + corp["mutated"]


def _auth(oracle, hostcheck, signers, use_list, once, max_keys=16, engine=WireListOracleEngine):
    a = _register(_Raising(engine=engine(oracle, hostcheck), max_keys=max_keys), signers)
    a._g.wire_list, a._g.wire_once = use_list or once, once
    return a


def _host_definition(oracle, signers, entries, max_keys):
    plain = _register(_Raising(engine=OracleEngine(oracle), max_keys=max_keys), signers)
    return plain._node_wire_decoded(entries)


def _assert_all_settings(oracle, hostcheck, signers, entries, max_keys):
    want = _host_definition(oracle, signers, entries, max_keys)
    auths = []
    for use_list, once in SETTINGS:
        a = _auth(oracle, hostcheck, signers, use_list, once, max_keys)
        got = a.authenticate_node_wire_batch(entries)
        assert [len(g) for g in got] == [len(w) for w in want]
        for e, (g, w) in enumerate(zip(got, want)):
            for x, y in zip(g, w):
                assert _same(x, y), (use_list, once, e, x, y)
        auths.append(a)
    base = auths[0]
    for a in auths[1:]:
        assert {k: a.stats[k] for k in EXISTING} == {k: base.stats[k] for k in EXISTING}
        assert a.seen == base.seen
    assert base.stats["wire_list_batches"] == 0 and base.stats["wire_distinct_items"] == 0
    assert base.engine.wire_list_calls == 0 and base.engine.wire_verifies >= 1
    for a in auths[1:]:
        # every verify of the wire path went through the list: not one per-item call
        assert a.engine.wire_verifies == 0
        assert a.stats["wire_list_batches"] == a.engine.wire_list_calls > 0
        assert a.stats["wire_distinct_items"] == a.engine.wire_list_lanes
    return auths


@pytest.mark.parametrize("max_keys", [16, 2])
def test_the_mixed_drain(oracle, hostcheck, drain, max_keys):
    signers, reqs, entries, _ = drain
    cls = [wum.unwrap(b, e)[0] for b, e in wum.messages(entries)]
    assert cls.count(wum.NONE) == 40 and cls.count(wum.HOST) == 1
    off, listed, once, both = _assert_all_settings(oracle, hostcheck, signers, entries, max_keys)
    # the live items: scanned, and their identifier has a 32-byte key (the signers 0 - 3)
    live = [i for i in range(len(reqs)) if i % 8 < 4]
    copies = sum(1 if i < 3 else 3 for i in live) - 1  # (request 19's first copy is the \u member)
    assert listed.stats["wire_distinct_items"] == copies
    assert listed.stats["batch_items"] == copies + 1  # (and the \u member through authenticate_batch)
    assert once.stats["wire_distinct_items"] == both.stats["wire_distinct_items"] == len(live)
    assert once.engine.last_give_ups == 0
    if max_keys == 16:
        assert off.stats["keyed_items"] == off.stats["batch_items"]
    else:  # two slots for four keys: some identifiers take the general path
        assert 0 < off.stats["keyed_items"] < off.stats["batch_items"]


def test_the_corpus(oracle, hostcheck, drain):
    signers, _, entries, corpus = drain
    mixed = corpus + entries
    random.Random(6).shuffle(mixed)
    _assert_all_settings(oracle, hostcheck, signers, mixed, 16)


def test_a_steady_drain_takes_the_list_only_with_once(oracle, hostcheck, drain):
    """Every message a scanned request with a registered key: the steady branch stays
    wire_verify_idents' unless each distinct request is to be verified once."""
    from plenum_amd.nodeloop import batch_text, propagate_text
    signers, _, _, _ = drain
    r = random.Random(3)
    reqs = []
    for i in range(40):
        d = wire_model.nym_dict(r, i)
        d["identifier"] = signers[i % 4].idr
        d["signature"] = wire_model.b58(signers[i % 4].sign(d))
        reqs.append(d)
    entries = [batch_text([propagate_text(d, "c%d" % i) for i, d in enumerate(reqs)]).encode()] * 3
    want = _host_definition(oracle, signers, entries, 16)
    seen = {}
    for use_list, once in SETTINGS:
        a = _auth(oracle, hostcheck, signers, use_list, once)
        got = a.authenticate_node_wire_batch(entries)
        assert all(_same(x, y) for g, w in zip(got, want) for x, y in zip(g, w)) and len(got) == len(want)
        assert all(x.__class__ is str for g in got for x in g)
        seen[(use_list, once)] = (a.engine.wire_list_calls, a.engine.wire_verify_idents_calls,
                                  a.stats["wire_distinct_items"], {k: a.stats[k] for k in EXISTING})
    assert seen[(False, False)][:3] == seen[(True, False)][:3] == (0, 1, 0)
    assert seen[(False, True)][:3] == seen[(True, True)][:3] == (1, 0, 40)
    assert len({str(v[3]) for v in seen.values()}) == 1 and seen[(True, True)][3]["batch_items"] == 120


def test_an_engine_without_the_list_behaves_as_before(oracle, hostcheck, drain):
    signers, _, entries, _ = drain
    a = _auth(oracle, hostcheck, signers, True, True, engine=WireSplitOracleEngine)
    assert not getattr(a.engine, "supports_wire_list", False)
    got = a.authenticate_node_wire_batch(entries)
    want = _host_definition(oracle, signers, entries, 16)
    assert all(_same(x, y) for g, w in zip(got, want) for x, y in zip(g, w))
    assert a.engine.wire_verifies == 1 and a.stats["wire_list_batches"] == 0


def test_the_switches_are_read_when_the_authenticator_is_made(oracle, monkeypatch):
    from plenum_amd.client_authn import GpuAuthNr
    for env, want in (({}, None), ({"EDV_WIRE_LIST": "1"}, (True, False)), ({"EDV_WIRE_ONCE": "1"}, (True, True)),
                      ({"EDV_WIRE_LIST": "0", "EDV_WIRE_ONCE": "0"}, (False, False)),
                      ({"EDV_WIRE_LIST": "0", "EDV_WIRE_ONCE": "1"}, (True, True))):
        for k in ("EDV_WIRE_LIST", "EDV_WIRE_ONCE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = GpuAuthNr(engine=OracleEngine(oracle))._g
        if want is None:  # the shipped defaults: once implies the list
            assert g.wire_list or not g.wire_once
        else:
            assert (g.wire_list, g.wire_once) == want


def test_wire_authenticate_takes_the_list_too(oracle, hostcheck, drain):
    """authenticate_wire_batch (client texts) off the steady state."""
    import json
    signers, reqs, _, _ = drain
    texts = [json.dumps(d).encode() for d in reqs[:64]] * 2 + [b"{}", b"nul"]
    want = _register(_Raising(engine=OracleEngine(oracle)), signers)._wire_decoded(texts, range(len(texts)), [None] * len(texts))
    for use_list, once in SETTINGS[1:]:
        a = _auth(oracle, hostcheck, signers, use_list, once)
        got = a.authenticate_wire_batch(texts)
        assert all(_same(x, y) for x, y in zip(got, want)) and len(got) == len(want)
        assert a.engine.wire_verifies == 0 and a.stats["wire_list_batches"] == 1
        live = [i for i in range(64) if i % 8 < 4]
        assert a.stats["wire_distinct_items"] == (len(live) if once else 2 * len(live))
