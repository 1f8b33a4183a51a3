"""Request digests from the wire batch, on the host: the digest pass's CPU twin (csrc/wire_digest.h
through libedv_hostcheck.so) against the Python definition -- which items it hashes, and what
it returns for them -- and authenticate_wire_batch / authenticate_node_wire_batch with
digests=True over wire_digest_double's engines."""
import itertools
import json
import random

import numpy as np
import pytest

import wire_digest_double as wdd
import wire_model
from engine_double import OracleEngine
from plenum_amd.batching import requests_in_drain
from plenum_amd.client_authn import GpuAuthNr, ReqAuthenticator
from plenum_amd.nodeloop import batch_text, propagate_text
from test_wire_authn import _Raising, _Signer, _register, _same
from wire_double import WireOracleEngine
from wire_node_double import WireNodeOracleEngine


def _twin(hostcheck, texts, base=0):
    buf, off = wire_model.pack_texts(texts, base)
    status, _, _, msgs, mlen = wire_model.twin_scan(hostcheck, buf, off)
    dig, have = wdd.twin_digests(hostcheck, buf, off, status, msgs, mlen)
    return status, dig, have


def _check_against_definition(texts, status, dig, have):
    """Every item of a twin run against the rule and the definition; (eligible, not eligible)
    among the status-0 items."""
    yes = no = 0
    for i, t in enumerate(texts):
        if status[i] != 0:
            assert not have[i] and not dig[i].any(), (i, t)
            continue
        d = json.loads(t)
        assert bool(have[i]) == wdd.eligible(d), (i, t)
        if have[i]:
            assert dig[i].tobytes() == wdd.definition(d), (i, t)
            yes += 1
        else:
            assert not dig[i].any(), (i, t)
            no += 1
    return yes, no


def test_twin_equals_the_definition_over_the_corpus(hostcheck):
    texts = wire_model.corpus()
    status, dig, have = _twin(hostcheck, texts)
    yes, no = _check_against_definition(texts, status, dig, have)
    assert yes >= 1000 and no >= 150, (yes, no)  # (the Python model alone: 1,377 and 235)
    assert int(np.count_nonzero(status)) >= 1500
    # the same texts at an odd place in their buffer
    status7, dig7, have7 = _twin(hostcheck, texts, base=7)
    assert (status7 == status).all() and (have7 == have).all() and (dig7 == dig).all()


# ------------------------------------------------------------------ hand-written walker edges
_SIG = wire_model._rand_sig(random.Random(5))
_BASE = [("identifier", '"L5AD5g65TDQr1PPHHRoiGf"'), ("reqId", "17"), ("operation", '{"type":"1","dest":"x"}'),
         ("protocolVersion", "2"), ("signature", '"%s"' % _SIG)]
_WS = " \t\n\r"


def _text(members, sep=",", colon=":", lead="", trail=""):
    return (lead + "{" + sep.join('"%s"%s%s' % (k, colon, v) for k, v in members) + "}" + trail).encode()


def _with(**changes):
    """_BASE with members replaced (None: left out); keys not in _BASE are appended."""
    out = [(k, changes.get(k, v)) for k, v in _BASE if changes.get(k, v) is not None]
    return out + [(k, v) for k, v in changes.items() if k not in dict(_BASE)]


def _edge_cases():
    """(name, text, eligible -- None: whatever the scan and the rule make of it)."""
    c = [("base", _text(_BASE), True)]
    for key in ("reqId2", "reqI", "Operation", "operation ", ""):
        c.append(("near-miss key %r added" % key, _text(_BASE + [(key, "1")]), False))
    c.append(("reqId2 for reqId", _text(_with(reqId=None, reqId2="1")), False))
    c.append(("reqI for reqId", _text(_with(reqId=None, reqI="1")), False))
    c.append(("Operation for operation", _text(_with(operation=None, Operation="{}")), False))
    nested = '{"identifier":"a","reqId":1,"operation":{"zz":1},"protocolVersion":null,"signature":"s","zz":[{"reqId":2}]}'
    c.append(("the names nested in operation", _text(_with(operation=nested)), True))
    c.append(("the names nested in operation, no protocolVersion", _text(_with(operation=nested, protocolVersion=None)),
              True))
    c.append(("the names nested, reqId only there", _text(_with(operation=nested, reqId=None)), False))
    c.append(("the names nested, operation only there", _text(_with(reqId=nested, operation=None)), False))
    objs = '[{"protocolVersion":null,"zz":1},{"reqId":2,"operation":null},[{"signature":"s"}]]'
    c.append(("the names in an array of objects (operation)", _text(_with(operation=objs)), True))
    c.append(("the names in an array of objects (protocolVersion)", _text(_with(protocolVersion=objs)), True))
    c.append(("the names in an array of objects, no reqId", _text(_with(operation=objs, reqId=None)), False))
    c.append(("protocolVersion null", _text(_with(protocolVersion="null")), False))
    c.append(("protocolVersion null, whitespace around the colon",
              b'{"protocolVersion" \n\t:\r\n null \n,' + _text(_with(protocolVersion=None))[1:], False))
    c.append(("protocolVersion null last", _text(_with(protocolVersion=None) + [("protocolVersion", " null ")]), False))
    c.append(('protocolVersion "null"', _text(_with(protocolVersion='"null"')), True))
    c.append(("protocolVersion 0", _text(_with(protocolVersion="0")), True))
    c.append(("protocolVersion false", _text(_with(protocolVersion="false")), True))
    c.append(("protocolVersion {}", _text(_with(protocolVersion="{}")), None))
    c.append(("protocolVersion absent", _text(_with(protocolVersion=None)), True))
    c.append(("reqId null", _text(_with(reqId="null")), True))
    c.append(("operation null", _text(_with(operation="null")), True))
    c.append(("reqId absent", _text(_with(reqId=None)), False))
    c.append(("operation absent", _text(_with(operation=None)), False))
    punct = r'{"a":"{}[]:,","b":"q\"uote","c":"ends\\","d":"\\\",\"zz\":\"","e":["]","}"]}'
    c.append(("punctuation and escapes in strings", _text(_with(operation=punct)), True))
    c.append(("punctuation and escapes, then an extra key", _text(_with(operation=punct, zz='"\\\\"')), False))
    c.append(("a string ending in a backslash, then protocolVersion null",
              _text(_with(operation=r'"ends\\"', protocolVersion=None) + [("protocolVersion", "null")]), False))
    c.append(("a key's text inside a string value", _text(_with(operation=r'"\",\"zz\":1,\"protocolVersion\":null"')),
              True))
    inner = "{" + _WS + '"type"' + _WS + ":" + _WS + '"1"' + _WS + "," + _WS + '"l"' + _WS + ":" + _WS + "[" + _WS + "1" + \
        _WS + "," + _WS + "null" + _WS + "]" + _WS + "}"
    spaced = [(k, inner if k == "operation" else v) for k, v in _BASE]
    c.append(("all four kinds of whitespace between every pair of tokens",
              (_WS + "{" + ",".join(_WS + '"%s"' % k + _WS + ":" + _WS + v + _WS for k, v in spaced) + "}" + _WS).encode(),
              True))
    r = random.Random(3)
    for k in range(6):
        order = list(_BASE)
        r.shuffle(order)
        c.append(("order %d" % k, _text(order), True))
        nul = [(a, "null" if a == "protocolVersion" else b) for a, b in order]
        c.append(("order %d, protocolVersion null" % k, _text(nul), False))
        c.append(("order %d, an extra key" % k, _text(order[:k % 5] + [("endorser", '"e"')] + order[k % 5:]), False))
    for first in itertools.permutations(range(5), 2):  # every pair of names first and second
        rest = [m for j, m in enumerate(_BASE) if j not in first]
        c.append(("order %d%d" % first, _text([_BASE[first[0]], _BASE[first[1]]] + rest, sep=", ", colon=": "), True))
    return c


def test_walker_edges(hostcheck):
    cases = _edge_cases()
    texts = [t for _, t, _ in cases]
    status, dig, have = _twin(hostcheck, texts)
    for (name, t, want), st in zip(cases, status):
        if want is not None:
            assert st == 0, (name, t)  # inside the scanner's grammar: the case tests the walk
            assert wdd.eligible(json.loads(t)) == want, (name, t)  # the case is what its name says
    _check_against_definition(texts, status, dig, have)
    for (name, t, _), st, h in zip(cases, status, have):
        if st == 0:
            assert wdd.twin_eligible(hostcheck, t) == int(h), (name, t)
    assert int(have.sum()) >= 30 and int((~have).sum()) >= 25


def test_walker_stops_at_the_end_of_a_truncated_text(hostcheck):
    """Every prefix of an eligible request through the walk alone: the asserted accessor aborts
    on a read at or past the prefix's length; only the whole text is eligible."""
    for t in (_text(_BASE), _text(_with(operation=r'{"a":"ends\\","b":[1,{"c":"\""}]}'), sep=" , ", colon=" : ",
                                  trail=" \n")):
        whole = len(t.rstrip())
        for cut in range(len(t) + 1):
            assert wdd.twin_eligible(hostcheck, t[:cut]) == int(cut >= whole), cut


# ------------------------------------------------------------------ the Python layer
def _signed_requests(oracle, signers, count, seed):
    """Signed NYM request dicts: every third forged; signers known, under a full key, with a None
    verkey, raising, unknown; some with a float (the host's grammar), some accepted but not
    eligible (another top-level key, no reqId, a null protocolVersion -- all covered by the
    signature)."""
    r = random.Random(seed)
    reqs = []
    for i in range(count):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        if i % 11 == 0:
            d["operation"]["amount"] = 1.5
        if i % 7 == 1:
            d["taaAcceptance"] = {"mechanism": "m", "time": 5}
        if i % 17 == 2:
            del d["reqId"]
        if i % 19 == 4:
            d["protocolVersion"] = None
        if i % 23 == 5:
            del d["protocolVersion"]
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        reqs.append(d)
    return reqs


@pytest.fixture(scope="module")
def signers(oracle):
    return [_Signer(oracle, k) for k in range(8)]


@pytest.fixture(scope="module")
def mixed_texts(oracle, signers):
    r = random.Random(8)
    texts = [wire_model.render(r, d) for d in _signed_requests(oracle, signers, 240, 21)]
    corpus = wire_model.corpus()
    texts += corpus[400:700] + corpus[-300:]
    r.shuffle(texts)
    return texts


@pytest.fixture(scope="module")
def mixed_entries(oracle, signers):
    reqs = _signed_requests(oracle, signers, 200, 22)
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(reqs)]
    prepare = json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 3, "digest": "d", "txnRootHash": None})
    entries = [json.dumps(d) for d in reqs[:30]] + props[30:60]
    for k in range(60, 180, 40):
        entries.append(batch_text(props[k:k + 20] + [prepare] + props[k + 20:k + 40] + [prepare]))
    entries += [batch_text([]), prepare, "not json {",
                batch_text([props[180].replace("client180", "client\\u0031"), props[181], prepare]),
                batch_text([batch_text(props[182:186]), props[186]])]
    punct = dict(reqs[1])  # BATCH members whose bodies are escaped twice over
    punct["operation"] = dict(punct["operation"], alias='q"uo\\te/ {}[]:,')
    punct["signature"] = wire_model.b58(signers[1].sign(punct))
    entries.append(batch_text([propagate_text(punct, "c\"x"), json.dumps(punct)] + props[187:200]))
    entries = [e.encode() for e in entries]
    random.Random(2).shuffle(entries)
    return entries


def _expected_split(hostcheck, results, texts_of_results):
    """(on the GPU, on the host) for the digest double: an accepted result is the GPU's when its
    text scanned (status 0) and is eligible."""
    accepted = [i for i, r in enumerate(results) if not isinstance(r, Exception)]
    status = wire_model.twin_scan(hostcheck, *wire_model.pack_texts([texts_of_results[i] for i in accepted]))[0]
    gpu = sum(1 for i, st in zip(accepted, status) if st == 0 and wdd.eligible(json.loads(texts_of_results[i])))
    return gpu, len(accepted) - gpu


def test_wire_batch_digests(oracle, hostcheck, signers, mixed_texts):
    texts = mixed_texts
    decoded = [wdd.loads_or_none(t) for t in texts]
    a = _register(_Raising(engine=wdd.WireDigestOracleEngine(oracle, hostcheck)), signers)
    results, digest, have = a.authenticate_wire_batch(texts, digests=True)
    accepted = wdd.check_contract(results, digest, have, decoded)
    gpu, host = _expected_split(hostcheck, results, texts)
    assert accepted >= 60 and gpu >= 40 and host >= 15, (accepted, gpu, host)
    st = a.stats
    assert (st["wire_digest_gpu"], st["wire_digest_host"]) == (gpu, host)
    assert a.engine.wire_digest_calls == 1 and a.engine.wire_scans == 1
    kinds = {type(r).__name__ for r in results}
    assert {"str", "InvalidSignature", "UnknownIdentifier", "JSONDecodeError"} <= kinds, kinds
    # the default returns what it returned before: the list alone, no digest pass
    b = _register(_Raising(engine=wdd.WireDigestOracleEngine(oracle, hostcheck)), signers)
    plain = b.authenticate_wire_batch(texts)
    assert type(plain) is list and len(plain) == len(texts)
    assert all(_same(p, r) for p, r in zip(plain, results))
    assert b.engine.wire_digest_calls == 0 and b.stats["wire_digest_gpu"] == b.stats["wire_digest_host"] == 0
    # an engine without the digest pass, and one without the wire path: the same triple
    for make in (lambda: WireOracleEngine(oracle, hostcheck), lambda: OracleEngine(oracle)):
        c = _register(_Raising(engine=make()), signers)
        res_c, digest_c, have_c = c.authenticate_wire_batch(texts, digests=True)
        assert all(_same(p, r) for p, r in zip(res_c, results)) and len(res_c) == len(results)
        assert (digest_c == digest).all() and (have_c == have).all()
        assert digest_c.dtype == np.uint8 and have_c.dtype == bool
        assert (c.stats["wire_digest_gpu"], c.stats["wire_digest_host"]) == (0, accepted)


def test_node_wire_batch_digests(oracle, hostcheck, signers, mixed_entries):
    entries = mixed_entries
    reqs = requests_in_drain(entries)
    a = _register(_Raising(engine=wdd.WireDigestNodeOracleEngine(oracle, hostcheck)), signers)
    out, digest, have = a.authenticate_node_wire_batch(entries, digests=True)
    assert [len(o) for o in out] == [len(requests_in_drain([e])) for e in entries]
    flat = [x for o in out for x in o]
    assert len(flat) == len(reqs) >= 200
    accepted = wdd.check_contract(flat, digest, have, reqs)
    gpu, host = _expected_split(hostcheck, flat, [json.dumps(d).encode() for d in reqs])
    assert accepted >= 50 and gpu >= 30 and host >= 10, (accepted, gpu, host)
    st = a.stats
    assert st["wire_digest_gpu"] + st["wire_digest_host"] == accepted
    # (a request reached through a message the unwrap left to the host is hashed on the host too)
    assert st["wire_digest_host"] >= host and 0 < st["wire_digest_gpu"] <= gpu
    assert a.engine.wire_digest_calls == 1 and a.engine.node_scans == 1
    b = _register(_Raising(engine=wdd.WireDigestNodeOracleEngine(oracle, hostcheck)), signers)
    plain = b.authenticate_node_wire_batch(entries)
    assert type(plain) is list and [len(p) for p in plain] == [len(o) for o in out]
    assert all(_same(p, r) for p, r in zip([x for o in plain for x in o], flat))
    assert b.engine.wire_digest_calls == 0
    for make in (lambda: WireNodeOracleEngine(oracle, hostcheck), lambda: OracleEngine(oracle)):
        c = _register(_Raising(engine=make()), signers)
        out_c, digest_c, have_c = c.authenticate_node_wire_batch(entries, digests=True)
        assert [len(o) for o in out_c] == [len(o) for o in out]
        assert all(_same(p, r) for p, r in zip([x for o in out_c for x in o], flat))
        assert (digest_c == digest).all() and (have_c == have).all()
        assert (c.stats["wire_digest_gpu"], c.stats["wire_digest_host"]) == (0, accepted)


def test_empty_inputs_other_inputs_and_the_aggregator(oracle, hostcheck, signers, mixed_texts, mixed_entries):
    a = _register(GpuAuthNr(engine=wdd.WireDigestNodeOracleEngine(oracle, hostcheck)), signers)
    for res, digest, have in (a.authenticate_wire_batch([], digests=True),
                              a.authenticate_node_wire_batch([], digests=True)):
        assert res == [] and digest.shape == (0, 32) and have.shape == (0,)
        assert digest.dtype == np.uint8 and have.dtype == bool
    out, digest, have = a.authenticate_node_wire_batch([batch_text([]).encode()] * 3, digests=True)
    assert out == [[], [], []] and digest.shape == (0, 32) and have.shape == (0,)
    few = mixed_texts[:80]
    want = a.authenticate_wire_batch(few, digests=True)
    ra = ReqAuthenticator()
    ra.register_authenticator(a)
    for got in (a.authenticate_wire_batch(tuple(few), digests=True),  # not a list: the host definition
                ra.authenticate_wire_batch(few, digests=True)):
        assert all(_same(p, r) for p, r in zip(got[0], want[0])) and len(got[0]) == len(few)
        assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
    assert type(ra.authenticate_wire_batch(few)) is list
    some = mixed_entries[:12]
    want = a.authenticate_node_wire_batch(some, digests=True)
    got = ra.authenticate_node_wire_batch(some, digests=True)
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all() and want[2].any()
    assert type(ra.authenticate_node_wire_batch(some)) is list
