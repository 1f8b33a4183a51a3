"""The wire path on the MI355X: edv_wire_scan_kernel against its CPU twin byte for byte
(through edv_wire_readback), edv_wire_verify against the C oracle, and
authenticate_wire_batch against authenticate_batch on a GpuAuthNr."""
import contextlib
import json
import random

import numpy as np
import pytest

import wire_model
from engine_double import OracleEngine

pytestmark = pytest.mark.gpu

NO_ID, SKIP = 0xFFFFFFFF, 0xFFFFFFFE


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


def _check_against_twin(eng, hostcheck, texts, base):
    buf, off = wire_model.pack_texts(texts, base=base)
    status, span = eng.wire_scan(buf, off)
    sig, msgs, mlen = eng.wire_readback()
    t_status, t_span, t_sig, t_msgs, t_mlen = wire_model.twin_scan(hostcheck, buf, off)
    assert status.tolist() == t_status.tolist()
    assert span.tolist() == t_span.tolist()
    assert mlen.tolist() == t_mlen.tolist()
    ok = np.flatnonzero(status == 0)
    assert (sig[ok] == t_sig[ok]).all()
    for i in ok.tolist():
        a = int(off[i] - off[0])
        assert msgs[a:a + int(mlen[i])].tobytes() == t_msgs[a:a + int(t_mlen[i])].tobytes(), (i, texts[i])
    return status


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096])
def test_scan_equals_cpu_twin(gpu_engine, hostcheck, n):
    """Shuffled corpus texts: 10-byte and 4 KiB items share an LDS tile, over-long items sit
    between scanned ones.  At 253 bytes a text on average the 64 items of a workgroup always end
    inside its first tile (tests/test_wire_tile_layouts.py asserts it); the second tile and the
    tile edges are tests/test_gpu_wire_tiles.py's."""
    r = random.Random(100 + n)
    texts = r.choices(wire_model.corpus(), k=n)
    status = _check_against_twin(gpu_engine, hostcheck, texts, 0)
    if n == 4096:
        assert (status == 0).sum() >= 1000 and (status == 1).sum() >= 1000


def test_scan_with_an_odd_base_offset_and_a_second_batch(gpu_engine, hostcheck):
    r = random.Random(5)
    _check_against_twin(gpu_engine, hostcheck, r.choices(wire_model.corpus(), k=777), 7)
    # a second scan replaces the batch: other texts, another item count
    second = r.choices(wire_model.corpus(), k=130)
    _check_against_twin(gpu_engine, hostcheck, second, 1)
    sig, msgs, mlen = gpu_engine.wire_readback()
    assert sig.shape == (130, 64) and len(mlen) == 130 and len(msgs) == sum(len(t) for t in second)
    with pytest.raises(Exception) as ei:
        gpu_engine.wire_verify(np.full(777, SKIP, np.uint32))  # the first batch's item count
    assert getattr(ei.value, "code", None) == -1


@pytest.fixture(scope="module")
def nym_batch(gpu_engine):
    """4,096 NYM request texts over 8 GPU-signed keys, every third S corrupted:
    (pk[8, 32], identifiers, verkeys, dicts, texts, key index per item, sig64, sers)."""
    from plenum_amd import pack_messages
    from plenum_amd.serialization import serialize_msg_for_signing
    from plenum_amd.synth import nym_request, signer_seeds
    n, k = 4096, 8
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    vks = ["~" + wire_model.b58(bytes(p[16:])) for p in pk]
    r = random.Random(3)
    kidx = (np.arange(n) % k).astype(np.uint32)
    dicts = [nym_request(idrs[i % k], 1_500_000_000_000_000 + i, wire_model.b58(r.randbytes(16)),
                         "~" + wire_model.b58(r.randbytes(16)), alias="a%d" % i if i % 5 == 0 else None)
             for i in range(n)]
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    buf, off = pack_messages(sers)
    sig = gpu_engine.sign_batch(sk, kidx, buf, off)
    sig[::3, 40] ^= 1
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    texts = [wire_model.render(r, d) for d in dicts]
    return pk, idrs, vks, dicts, texts, kidx, sig, sers


@pytest.fixture(scope="module")
def nym_expect(oracle, nym_batch):
    """The C oracle's crypto_sign_open on sig || ser (computed once)."""
    from plenum_amd import pack_messages
    pk, _, _, _, _, kidx, sig, sers = nym_batch
    buf, off = pack_messages(sers)
    want = OracleEngine(oracle).verify_batch(sig, pk[kidx], buf, off)
    assert want.sum() == 4096 - len(range(0, 4096, 3))
    return want


def test_wire_verify_keyed_general_mixed_and_skipped(gpu_engine, nym_batch, nym_expect):
    pk, _, _, _, texts, kidx, _, _ = nym_batch
    buf, off = wire_model.pack_texts(texts)
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(pk)
        status, _ = gpu_engine.wire_scan(buf, off)
        assert not status.any()  # the model accepts every NYM text
        ids = (kidx + first).astype(np.uint32)
        none = np.full(len(texts), NO_ID, np.uint32)
        assert (gpu_engine.wire_verify(ids) == nym_expect).all()                      # all registered
        assert (gpu_engine.wire_verify(none, pk[kidx]) == nym_expect).all()          # none registered
        half = np.where(kidx % 2 == 0, ids, none).astype(np.uint32)
        assert (gpu_engine.wire_verify(half, pk[kidx]) == nym_expect).all()          # the mixed launch
        skipped = half.copy()
        skipped[5::7] = SKIP
        want = nym_expect.copy()
        want[5::7] = False
        assert (gpu_engine.wire_verify(skipped, pk[kidx]) == want).all()
        assert not gpu_engine.wire_verify(np.full(len(texts), SKIP, np.uint32)).any()
        unknown = ids.copy()
        unknown[::2] = first + 1000  # not a registered id: rejected, never read
        assert (gpu_engine.wire_verify(unknown) == (nym_expect & (np.arange(len(texts)) % 2 == 1))).all()


@pytest.mark.parametrize("max_keys", [16, 0])
def test_authenticate_wire_batch_equals_authenticate_batch(gpu_engine, nym_batch, nym_expect, max_keys):
    from plenum_amd.client_authn import GpuAuthNr
    _, idrs, vks, dicts, texts, kidx, _, _ = nym_batch
    with _own_keys(gpu_engine):
        wire, plain = (GpuAuthNr(engine=gpu_engine, max_keys=max_keys) for _ in range(2))
        for a in (wire, plain):
            for idr, vk in zip(idrs, vks):
                a.addIdr(idr, vk)
            a.keys_settle()
        got = wire.authenticate_wire_batch(texts)
        want = plain.authenticate_batch([json.loads(t) for t in texts])
        for i, (g, w) in enumerate(zip(got, want)):
            assert type(g) is type(w) and (g == w if isinstance(w, str) else g.args == w.args), (i, g, w)
            assert (g == idrs[kidx[i]]) == bool(nym_expect[i]), (i, g)
        st = wire.stats
        assert st["wire_host_items"] == 0 and st["wire_items"] == len(texts)
        assert st["keyed_items"] == (len(texts) if max_keys else 0)


def test_mixed_texts_through_the_authenticator(gpu_engine, nym_batch):
    """Scanned and host-decided texts in one batch, an unknown identifier, unparsable texts."""
    from plenum_amd.client_authn import GpuAuthNr
    _, idrs, vks, _, texts, _, _, _ = nym_batch
    r = random.Random(8)
    batch = texts[:300] + r.choices(wire_model.corpus(), k=700)
    r.shuffle(batch)
    with _own_keys(gpu_engine):
        wire, plain = (GpuAuthNr(engine=gpu_engine) for _ in range(2))
        for a in (wire, plain):
            for idr, vk in zip(idrs[:6], vks):
                a.addIdr(idr, vk)
            a.keys_settle()
        got = wire.authenticate_wire_batch(batch)
        idx, decoded, want = [], [], [None] * len(batch)
        for i, t in enumerate(batch):
            try:
                decoded.append(json.loads(t))
                idx.append(i)
            except ValueError as ex:
                want[i] = ex
        for i, res in zip(idx, plain.authenticate_batch(decoded)):
            want[i] = res
        for i, (g, w) in enumerate(zip(got, want)):
            assert type(g) is type(w), (i, batch[i], g, w)
            if isinstance(w, Exception):
                assert g.args == w.args and type(g.__cause__) is type(w.__cause__), (i, batch[i], g, w)
            else:
                assert g == w
        assert wire.stats["wire_items"] + wire.stats["wire_host_items"] == len(batch)
        assert wire.stats["wire_items"] >= 300 and wire.stats["wire_host_items"] >= 100


def test_fresh_context_and_the_resident_kernel(nym_batch, nym_expect):
    """wire_verify / wire_readback before any scan are EDV_EINVAL; a single request
    (edv_verify_one: the resident kernel) answers before and after a wire batch."""
    from plenum_amd import EdVerifyEngine
    pk, _, _, _, texts, kidx, sig, sers = nym_batch
    with EdVerifyEngine(0) as eng:
        for call in (lambda: eng.wire_verify(np.zeros(4, np.uint32)), eng.wire_readback):
            with pytest.raises(Exception) as ei:
                call()
            assert getattr(ei.value, "code", None) == -1
        first = eng.keys_add(pk)
        assert eng.verify_one_keyed(sig[1].tobytes(), first + int(kidx[1]), sers[1]) == bool(nym_expect[1])
        assert eng.verify_one_keyed(sig[0].tobytes(), first + int(kidx[0]), sers[0]) == bool(nym_expect[0])
        buf, off = wire_model.pack_texts(texts[:512])
        status, _ = eng.wire_scan(buf, off)
        assert not status.any()
        ok = eng.wire_verify((kidx[:512] + first).astype(np.uint32))
        assert (ok == nym_expect[:512]).all()
        for i in (2, 3, 4):
            assert eng.verify_one_keyed(sig[i].tobytes(), first + int(kidx[i]), sers[i]) == bool(nym_expect[i])
        status, _ = eng.wire_scan(*wire_model.pack_texts([]))
        assert len(status) == 0 and len(eng.wire_verify(np.zeros(0, np.uint32))) == 0
