"""The wire batch's distinct identifiers (csrc/wire_idents.h) on the CPU: the twin of the
edv_wire_ident_* kernels' lane code (libedv_hostcheck.so hc_wire_idents, every access asserted
in bounds) against _hostpack.wire_idents, in any insertion order and with a full table; and
authenticate_wire_batch over an engine with the identifier pass against one without."""
import json
import random

import numpy as np
import pytest

import wire_model
from plenum_amd import _hostpack
from plenum_amd.client_authn import GpuAuthNr
from test_wire_authn import _Raising, _Signer, _decoded_results, _register, _same
from wire_double import WireOracleEngine
from wire_idents_double import (HAND_MADE, HAND_NU, WireIdentsOracleEngine, ident_strings, minimal_text, pow2_at_least,
                                twin_idents)


def _scanned(hostcheck, texts, base=0):
    buf, off = wire_model.pack_texts(texts, base=base)
    status, span = wire_model.twin_scan(hostcheck, buf, off)[:2]
    return buf, off, status, span


def _host_pass(buf, off, status, span):
    uidx_b, uniq = _hostpack.wire_idents(buf, off.tobytes(), status, span)
    return np.frombuffer(uidx_b, np.uint32), uniq


def _check(hostcheck, batch, cap=None, order=None):
    """The twin over `batch` == the host pass; returns (uidx, uniq_item)."""
    buf, off, status, span = batch
    want_uidx, want_uniq = _host_pass(buf, off, status, span)
    nu, uidx, uniq_item = twin_idents(hostcheck, buf, off, status, span, cap, order)
    assert nu == len(want_uniq)
    assert uidx.tolist() == want_uidx.tolist()
    assert ident_strings(buf, off, span, uniq_item) == want_uniq
    return uidx, uniq_item


def _orders(n):
    yield np.arange(n)
    yield np.arange(n)[::-1]
    for seed in (1, 2, 3):
        yield np.random.default_rng(seed).permutation(n)


@pytest.fixture(scope="module")
def corpus_4096(hostcheck):
    return _scanned(hostcheck, random.Random(4196).choices(wire_model.corpus(), k=4096))


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4096])
def test_twin_equals_host_pass_on_corpus_batches(hostcheck, corpus_4096, n):
    batch = corpus_4096 if n == 4096 else _scanned(hostcheck, random.Random(100 + n).choices(wire_model.corpus(), k=n),
                                                   base=n % 5)
    status = batch[2]
    if n == 4096:
        assert (status == 0).sum() >= 1000 and (status == 1).sum() >= 1000  # scanned and host items mix
    uidx, uniq_item = _check(hostcheck, batch, cap=pow2_at_least(2 * n))
    nu = len(uniq_item)
    assert (uidx[status != 0] == nu).all() and (uidx[status == 0] < nu).all()
    _check(hostcheck, batch, cap=pow2_at_least(nu))  # as full as a table of a power of two gets


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_identifier_sets(hostcheck, name):
    batch = _scanned(hostcheck, HAND_MADE[name])
    if name != "only host items":
        assert not batch[2].any()  # the model accepts the minimal texts
    nu = HAND_NU[name]
    for cap in (None, pow2_at_least(nu)):
        for order in _orders(len(HAND_MADE[name])):
            uidx, uniq_item = _check(hostcheck, batch, cap, order)
            assert len(uniq_item) == nu
    if name == "only host items":
        assert batch[2].all() and not uidx.any()


def test_all_distinct_in_a_full_table(hostcheck):
    n = 4096
    batch = _scanned(hostcheck, [minimal_text("did:%d" % (i * 7919 % n)) for i in range(n)])
    assert not batch[2].any()
    for order in _orders(n):
        uidx, uniq_item = _check(hostcheck, batch, cap=n, order=order)  # every slot taken: the chains wrap
        assert uidx.tolist() == list(range(n)) and uniq_item.tolist() == list(range(n))
    assert twin_idents(hostcheck, *batch, cap=n // 2)[0] == -2  # (a table too small is refused, not looped in)


def test_any_insertion_order_gives_the_same_result(hostcheck, corpus_4096):
    first = None
    for order in _orders(4096):
        uidx, uniq_item = _check(hostcheck, corpus_4096, order=order)
        got = (uidx.tolist(), uniq_item.tolist())
        first = first or got
        assert got == first
    nu = len(first[1])
    for order in _orders(4096):
        uidx, uniq_item = _check(hostcheck, corpus_4096, cap=pow2_at_least(nu), order=order)
        assert (uidx.tolist(), uniq_item.tolist()) == first


def test_a_span_past_its_item_is_refused_unread(hostcheck):
    texts = [minimal_text("abc"), minimal_text("abd"), minimal_text("abc")]
    buf, off, status, span = _scanned(hostcheck, texts)
    assert twin_idents(hostcheck, buf, off, status, span)[0] == 2
    for item, start, length in ((0, None, len(texts[0])),           # into the next item
                                (2, None, len(texts[2])),           # past the end of the buffer
                                (1, len(texts[1]), 1), (1, len(texts[1]) + 1, 0),
                                (2, 0xFFFFFFFF, 0xFFFFFFFF), (2, 0xFFFFFFFF, 2), (0, 3, 0xFFFFFFFE)):
        bad = span.copy()
        if start is not None:
            bad[item, 0] = start
        bad[item, 1] = length
        # (the asserted accessors abort the process on a read outside the texts: returning shows none)
        assert twin_idents(hostcheck, buf, off, status, bad)[0] == -1
    edge = span.copy()
    edge[1] = (len(texts[1]), 0)  # an empty span at the very end of its item is inside it
    nu, uidx, uniq_item = twin_idents(hostcheck, buf, off, status, edge)
    assert nu == 2 and uidx.tolist() == [0, 1, 0] and ident_strings(buf, off, edge, uniq_item) == ["abc", ""]
    host = status.copy()
    host[2] = 1  # a bad span of an item the host decides is never looked at
    bad = span.copy()
    bad[2] = (0xFFFFFFFF, 0xFFFFFFFF)
    assert twin_idents(hostcheck, buf, off, host, bad)[0] == 2


# ---------------------------------------------------------------- the authenticator on the CPU
def _pair(oracle, hostcheck, cls, register, monkeypatch):
    monkeypatch.setenv("EDV_WIRE_IDENTS", "1")  # (read when the authenticator is made)
    new = register(cls(engine=WireIdentsOracleEngine(oracle, hostcheck)))
    old = register(cls(engine=WireOracleEngine(oracle, hostcheck)))
    assert new._g.wire_idents_gpu
    return new, old


@pytest.fixture(scope="module")
def signed_texts(oracle):
    """About 2,000 texts: signed NYM requests over 8 signers (known by an abbreviated or a full
    verkey, with a None verkey, unknown, or whose getVerkey raises; every third S corrupted; a
    float that sends the item to the host) and corpus texts."""
    r = random.Random(14)
    signers = [_Signer(oracle, k) for k in range(8)]
    texts = []
    for i in range(320):
        s = signers[i % 8]
        d = wire_model.nym_dict(r, i)
        kind = i % 8
        d["identifier"] = {5: "full-key-%d" % kind, 6: "boom-%d" % (i % 3), 7: "nobody-%d" % (i % 5)}.get(kind, s.idr)
        if i % 11 == 0:
            d["operation"]["amount"] = 1.5
        sig = bytearray(s.sign(d))
        if i % 3 == 0:
            sig[40] ^= 1
        d["signature"] = wire_model.b58(bytes(sig))
        texts.append(wire_model.render(r, d))
    corpus = wire_model.corpus()
    texts += corpus[300:300 + 900] + corpus[-800:]
    r.shuffle(texts)
    return signers, texts


def test_authenticator_with_the_identifier_pass_equals_the_host_pass(oracle, hostcheck, signed_texts, monkeypatch):
    signers, texts = signed_texts
    new, old = _pair(oracle, hostcheck, _Raising, lambda a: _register(a, signers), monkeypatch)
    got, want = new.authenticate_wire_batch(texts), old.authenticate_wire_batch(texts)
    assert len(got) == len(want) == len(texts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (i, texts[i], g, w)
    kinds = {type(w).__name__ for w in want}
    assert {"str", "InvalidSignature", "UnknownIdentifier", "CouldNotAuthenticate", "JSONDecodeError"} <= kinds, kinds
    assert new.seen == old.seen and len(new.seen) > 20  # getVerkey: the same calls in the same order
    assert new.stats == old.stats
    assert new.stats["wire_items"] >= 500 and new.stats["wire_host_items"] >= 300
    eng = new.engine
    assert eng.wire_idents_calls == 1 and eng.wire_verify_idents_calls == 0 and eng.wire_verifies == 1
    # ... and both equal the dict path over the decoded texts
    plain = _register(_Raising(engine=WireOracleEngine(oracle, hostcheck)), signers)
    for i, (g, w) in enumerate(zip(got, _decoded_results(plain, texts))):
        assert _same(g, w), (i, texts[i], g, w)


def test_unknown_identifier_and_raising_getverkey_among_scanned_items(oracle, hostcheck, signed_texts, monkeypatch):
    signers, texts = signed_texts
    scanned = [t for t in texts if wire_model.scan(t) is not None]
    status = wire_model.twin_scan(hostcheck, *wire_model.pack_texts(scanned))[0]
    scanned = [t for t, s in zip(scanned, status) if s == 0]
    assert len(scanned) >= 400
    new, old = _pair(oracle, hostcheck, _Raising, lambda a: _register(a, signers), monkeypatch)
    got, want = new.authenticate_wire_batch(scanned), old.authenticate_wire_batch(scanned)
    assert all(_same(g, w) for g, w in zip(got, want))
    first_seen = list(dict.fromkeys(wire_model.scan(t)[1] for t in scanned))
    assert new.seen == old.seen == first_seen  # once each, in first-occurrence order
    assert any(s.startswith("boom") for s in first_seen) and any(s.startswith("nobody") for s in first_seen)
    assert new.stats == old.stats and new.stats["wire_host_items"] == 0


def test_steady_state_makes_one_wire_verify_idents_call(oracle, hostcheck, monkeypatch):
    r = random.Random(16)
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

    def register(a):
        for s in signers:
            a.addIdr(s.idr, s.abbreviated)
        a.keys_settle()
        return a
    new, old = _pair(oracle, hostcheck, GpuAuthNr, register, monkeypatch)
    got, want = new.authenticate_wire_batch(texts), old.authenticate_wire_batch(texts)
    assert all(_same(g, w) for g, w in zip(got, want))
    assert [isinstance(g, str) for g in got] == [i % 5 != 0 for i in range(200)]
    assert all(_same(g, w) for g, w in zip(got, register(GpuAuthNr(engine=WireOracleEngine(oracle, hostcheck)))
                                           .authenticate_batch([json.loads(t) for t in texts])))
    assert new.stats == old.stats
    assert new.stats["wire_items"] == new.stats["keyed_items"] == new.stats["batch_items"] == 200
    eng = new.engine
    assert eng.wire_idents_calls == 1 and eng.wire_verify_idents_calls == 1 and eng.wire_verifies == 0
    assert old.engine.wire_verifies == 1
    assert set(new._g.last_wire_breakdown) == set(old._g.last_wire_breakdown)


def test_the_environment_switch_selects_the_host_pass(oracle, hostcheck, monkeypatch):
    monkeypatch.setenv("EDV_WIRE_IDENTS", "0")
    a = GpuAuthNr(engine=WireIdentsOracleEngine(oracle, hostcheck))
    monkeypatch.setenv("EDV_WIRE_IDENTS", "1")
    assert not a._g.wire_idents_gpu
    texts = [minimal_text("nobody-%d" % (i % 3)) for i in range(10)]
    b = GpuAuthNr(engine=WireIdentsOracleEngine(oracle, hostcheck))
    assert all(_same(g, w) for g, w in zip(a.authenticate_wire_batch(texts), b.authenticate_wire_batch(texts)))
    assert a.engine.wire_idents_calls == 0 and b.engine.wire_idents_calls == 1
    assert a.stats == b.stats
