"""The wire batch's identifier pass on the MI355X: edv_wire_idents against the host pass
(_hostpack.wire_idents) element for element, edv_wire_verify_idents against edv_wire_verify and
the C oracle, the two calls' contract, and authenticate_wire_batch with the pass on and off."""
import contextlib
import json
import random

import numpy as np
import pytest

import wire_model
from engine_double import OracleEngine
from plenum_amd import _hostpack
from wire_idents_double import HAND_MADE, ident_strings, minimal_text

pytestmark = pytest.mark.gpu

SKIP = 0xFFFFFFFE


@contextlib.contextmanager
def _own_keys(eng):
    """The engine's key store emptied for the test and again after it."""
    eng.__dict__.pop("_edv_key_store", None)
    eng.keys_reset()
    try:
        yield
    finally:
        eng.__dict__.pop("_edv_key_store", None)
        eng.keys_reset()


def _check_against_host_pass(eng, texts, base=0):
    buf, off = wire_model.pack_texts(texts, base=base)
    status, span = eng.wire_scan(buf, off)
    uidx, uniq_item = eng.wire_idents()
    want_b, want_uniq = _hostpack.wire_idents(buf, off.tobytes(), status, span)
    assert uidx.dtype == np.uint32 and uniq_item.dtype == np.uint32
    assert len(uniq_item) == len(want_uniq)
    assert uidx.tolist() == np.frombuffer(want_b, np.uint32).tolist()
    assert ident_strings(buf, off, span, uniq_item) == want_uniq
    return status, uidx, uniq_item


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096])
def test_idents_equal_the_host_pass_on_corpus_batches(gpu_engine, n):
    texts = random.Random(100 + n).choices(wire_model.corpus(), k=n)
    status, uidx, uniq_item = _check_against_host_pass(gpu_engine, texts, base=n % 5)
    if n == 4096:
        assert (status == 0).sum() >= 1000 and (status == 1).sum() >= 1000
        assert (uidx[status != 0] == len(uniq_item)).all()


def test_idents_three_identifiers_contended(gpu_engine):
    r = random.Random(7)
    texts = [minimal_text("signer-%d" % r.randrange(3), r.randrange(4)) for _ in range(8192)]
    _, _, uniq_item = _check_against_host_pass(gpu_engine, texts)
    assert len(uniq_item) == 3


def test_idents_all_distinct(gpu_engine):
    n = 8192
    texts = [minimal_text("did:%d" % (i * 7919 % n)) for i in range(n)]
    _, uidx, uniq_item = _check_against_host_pass(gpu_engine, texts)
    assert uidx.tolist() == list(range(n)) and uniq_item.tolist() == list(range(n))
    pinned = gpu_engine.host_alloc(4 * n + 64)  # uidx copied straight into the caller's pinned memory
    view, uniq_again = gpu_engine.wire_idents(pinned)
    assert view.tolist() == list(range(n)) and uniq_again.tolist() == list(range(n))
    assert np.frombuffer(pinned, np.uint32, count=n).tolist() == list(range(n))


@pytest.mark.parametrize("name", ["prefix pair", "last byte", "only host items"])
def test_idents_hand_made_sets(gpu_engine, name):
    _check_against_host_pass(gpu_engine, HAND_MADE[name])


@pytest.fixture(scope="module")
def nym_batch(gpu_engine):
    """4,096 NYM request texts over 8 GPU-signed keys, every third S corrupted:
    (pk[8, 32], identifiers, verkeys, texts, key index per item, sig64, sers)."""
    from plenum_amd import pack_messages
    from plenum_amd.serialization import serialize_msg_for_signing
    from plenum_amd.synth import nym_request, signer_seeds
    n, k = 4096, 8
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    vks = ["~" + wire_model.b58(bytes(p[16:])) for p in pk]
    r = random.Random(13)
    kidx = np.array([r.randrange(k) for _ in range(n)], np.uint32)
    dicts = [nym_request(idrs[kidx[i]], 1_500_000_000_000_000 + i, wire_model.b58(r.randbytes(16)),
                         "~" + wire_model.b58(r.randbytes(16)), alias="a%d" % i if i % 5 == 0 else None)
             for i in range(n)]
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    buf, off = pack_messages(sers)
    sig = gpu_engine.sign_batch(sk, kidx, buf, off)
    sig[::3, 40] ^= 1
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    texts = [wire_model.render(r, d) for d in dicts]
    return pk, idrs, vks, texts, kidx, sig, sers


@pytest.fixture(scope="module")
def nym_expect(oracle, nym_batch):
    """The C oracle's crypto_sign_open on sig || ser of the first 512 (computed once)."""
    from plenum_amd import pack_messages
    pk, _, _, _, kidx, sig, sers = nym_batch
    buf, off = pack_messages(sers[:512])
    want = OracleEngine(oracle).verify_batch(sig[:512], pk[kidx[:512]], buf, off)
    assert want.sum() == 512 - len(range(0, 512, 3))
    return want


def test_verify_idents_equals_wire_verify_and_the_oracle(gpu_engine, nym_batch, nym_expect):
    pk, _, _, texts, kidx, _, _ = nym_batch
    buf, off = wire_model.pack_texts(texts[:512])
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(pk)
        status, _ = gpu_engine.wire_scan(buf, off)
        assert not status.any()
        uidx, uniq_item = gpu_engine.wire_idents()
        assert len(uniq_item) == 8 and (kidx[uniq_item][uidx] == kidx[:512]).all()
        kid_u = (kidx[uniq_item] + first).astype(np.uint32)
        got = gpu_engine.wire_verify_idents(kid_u)
        assert (got == gpu_engine.wire_verify(kid_u[uidx])).all()
        assert (got == nym_expect).all()
        assert (gpu_engine.wire_verify_idents(kid_u) == nym_expect).all()  # (uidx outlives a wire_verify)
        unknown = kid_u.copy()
        unknown[3] = first + 1000  # not a registered id: its items rejected, the call does not fail
        want = nym_expect & (uidx != 3)
        assert (uidx == 3).any()
        assert (gpu_engine.wire_verify_idents(unknown) == want).all()
        assert (gpu_engine.wire_verify(unknown[uidx]) == want).all()


def test_contract_of_the_two_calls(nym_batch, nym_expect):
    """Every misuse is EDV_EINVAL (-1) and leaves the context usable."""
    from plenum_amd import EdVerifyEngine
    pk, _, _, texts, kidx, _, _ = nym_batch

    def refused(call):
        with pytest.raises(Exception) as ei:
            call()
        assert getattr(ei.value, "code", None) == -1, ei.value

    good = wire_model.pack_texts(texts[:512])
    with EdVerifyEngine(0) as eng:
        refused(eng.wire_idents)                                        # a fresh context
        first = eng.keys_add(pk)
        eng.wire_scan(*good)
        refused(lambda: eng.wire_verify_idents(np.full(8, first, np.uint32)))   # before wire_idents
        uidx, uniq_item = eng.wire_idents()
        kid_u = (kidx[uniq_item] + first).astype(np.uint32)
        eng.wire_scan(*good)
        refused(lambda: eng.wire_verify_idents(kid_u))                  # the batch was rescanned since
        eng.wire_idents()
        refused(lambda: eng.wire_verify_idents(kid_u[:7]))              # a wrong n_uniq
        refused(lambda: eng.wire_verify_idents(np.append(kid_u, kid_u[:1])))
        skipped = kid_u.copy()
        skipped[2] = SKIP
        refused(lambda: eng.wire_verify_idents(skipped))                # not a key id
        mixed = wire_model.pack_texts(texts[:100] + [b'{"identifier":"idr","x":1.5}'] + texts[100:200])
        status, _ = eng.wire_scan(*mixed)
        assert status.sum() == 1
        uidx_m, uniq_m = eng.wire_idents()
        assert uidx_m[100] == len(uniq_m) == 8 and (uniq_m < 100).all()
        refused(lambda: eng.wire_verify_idents((kidx[uniq_m] + first).astype(np.uint32)))  # a host-status item
        # ... and the context goes on: a scan, idents and verify round with the right verdicts
        eng.wire_scan(*good)
        uidx2, uniq2 = eng.wire_idents()
        assert uidx2.tolist() == uidx.tolist() and uniq2.tolist() == uniq_item.tolist()
        assert (eng.wire_verify_idents(kid_u) == nym_expect).all()
        status, _ = eng.wire_scan(*wire_model.pack_texts([]))
        uidx0, uniq0 = eng.wire_idents()
        assert len(status) == len(uidx0) == len(uniq0) == 0
        assert len(eng.wire_verify_idents(np.zeros(0, np.uint32))) == 0


def _authenticators(gpu_engine, monkeypatch, idrs, vks):
    from plenum_amd.client_authn import GpuAuthNr
    out = []
    for env in ("1", "0"):
        monkeypatch.setenv("EDV_WIRE_IDENTS", env)  # (read when the authenticator is made)
        out.append(GpuAuthNr(engine=gpu_engine))
    plain = GpuAuthNr(engine=gpu_engine)
    monkeypatch.delenv("EDV_WIRE_IDENTS")
    assert out[0]._g.wire_idents_gpu and not out[1]._g.wire_idents_gpu
    for a in out + [plain]:
        for idr, vk in zip(idrs, vks):
            a.addIdr(idr, vk)
        a.keys_settle()
    return out[0], out[1], plain


def _counters(a):
    return {k: a.stats[k] for k in ("batches", "batch_items", "keyed_items", "wire_items", "wire_host_items")}


def _same(g, w):
    if isinstance(w, Exception):
        return type(g) is type(w) and g.args == w.args and type(g.__cause__) is type(w.__cause__)
    return type(g) is type(w) and g == w


def test_authenticate_wire_batch_with_the_pass_on_and_off(gpu_engine, nym_batch, monkeypatch):
    _, idrs, vks, texts, kidx, _, _ = nym_batch
    with _own_keys(gpu_engine):
        on, off, plain = _authenticators(gpu_engine, monkeypatch, idrs, vks)
        got_on, got_off = on.authenticate_wire_batch(texts), off.authenticate_wire_batch(texts)
        want = plain.authenticate_batch([json.loads(t) for t in texts])
        for i, (a, b, w) in enumerate(zip(got_on, got_off, want)):
            assert _same(a, w) and _same(b, w), (i, a, b, w)
        assert sum(isinstance(w, str) for w in want) == len(texts) - len(range(0, len(texts), 3))
        for a in (on, off):
            assert a.stats["wire_host_items"] == 0 and a.stats["wire_items"] == len(texts)
            assert a.stats["keyed_items"] == len(texts)
        assert _counters(on) == _counters(off)
        assert set(on._g.last_wire_breakdown) == set(off._g.last_wire_breakdown)


def test_mixed_texts_with_the_pass_on_and_off(gpu_engine, nym_batch, monkeypatch):
    """Scanned and host-decided texts in one batch, unknown identifiers, unparsable texts."""
    _, idrs, vks, texts, _, _, _ = nym_batch
    r = random.Random(18)
    batch = texts[:300] + r.choices(wire_model.corpus(), k=700)
    r.shuffle(batch)
    with _own_keys(gpu_engine):
        on, off, plain = _authenticators(gpu_engine, monkeypatch, idrs[:6], vks)
        got_on, got_off = on.authenticate_wire_batch(batch), off.authenticate_wire_batch(batch)
        idx, decoded, want = [], [], [None] * len(batch)
        for i, t in enumerate(batch):
            try:
                decoded.append(json.loads(t))
                idx.append(i)
            except ValueError as ex:
                want[i] = ex
        for i, res in zip(idx, plain.authenticate_batch(decoded)):
            want[i] = res
        for i, (a, b, w) in enumerate(zip(got_on, got_off, want)):
            assert _same(a, w) and _same(b, w), (i, batch[i], a, b, w)
        assert _counters(on) == _counters(off)
        assert on.stats["wire_items"] + on.stats["wire_host_items"] == len(batch)
        assert on.stats["wire_items"] >= 300 and on.stats["wire_host_items"] >= 100
