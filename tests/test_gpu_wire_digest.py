"""Request digests from the wire batch on the MI355X: edv_wire_digest_kernel against its CPU
twin (libedv_hostcheck.so hc_wire_digests) over whole output buffers, edv_wire_digests' call
order, and authenticate_wire_batch / authenticate_node_wire_batch with digests=True against
request_digests over the decoded requests."""
import contextlib
import json
import random

import numpy as np
import pytest

import wire_digest_double as wdd
import wire_model
from plenum_amd.serialization import serialize_msg_for_signing

pytestmark = pytest.mark.gpu

_SIG = wire_model._rand_sig(random.Random(5))


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


def _kernel_equals_twin(eng, hostcheck, texts, base=0):
    """One scan and one digest pass on the GPU against the twin's, every byte of both outputs."""
    buf, off = wire_model.pack_texts(texts, base)
    status, _ = eng.wire_scan(buf, off)
    dig, have = eng.wire_digests()
    assert dig.shape == (len(texts), 32) and dig.dtype == np.uint8 and have.dtype == bool
    t_status, _, _, msgs, mlen = wire_model.twin_scan(hostcheck, buf, off)
    assert (status == t_status).all()
    t_dig, t_have = wdd.twin_digests(hostcheck, buf, off, t_status, msgs, mlen)
    assert (have == t_have).all(), np.flatnonzero(have != t_have)[:8]
    assert (dig == t_dig).all(), np.flatnonzero((dig != t_dig).any(axis=1))[:8]
    assert not dig[~have].any()
    return status, dig, have


@pytest.mark.parametrize("base", [0, 13])
def test_corpus_as_one_batch(gpu_engine, hostcheck, base):
    status, _, have = _kernel_equals_twin(gpu_engine, hostcheck, wire_model.corpus(), base)
    assert int(have.sum()) >= 1000 and int((~have & (status == 0)).sum()) >= 150


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_last_partial_wave_and_block(gpu_engine, hostcheck, n):
    texts = random.Random(40 + n).choices(wire_model.corpus()[:1800], k=n)
    texts[-1] = wire_model.corpus()[0]  # (a NYM rendering: the last lane hashes)
    _, _, have = _kernel_equals_twin(gpu_engine, hostcheck, texts, base=n % 3)
    assert have[-1] and int(have.sum()) >= (n + 1) // 2


def _sized(ser_len, key="a"):
    """An eligible request text whose serialization is ser_len bytes (a string inside operation
    padded), and that serialization."""
    d = {"identifier": "i", "reqId": 1, "operation": {key: ""}, "signature": _SIG}
    d["operation"][key] = "x" * (ser_len - len(serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"])))
    ser = serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"])
    assert len(ser) == ser_len
    return json.dumps(d, separators=(",", ":")).encode(), ser


@pytest.mark.parametrize("align", [0, 1, 7, 8, 15])
def test_sha256_padding_edges_at_every_alignment(gpu_engine, hostcheck, align):
    """Serializations of 55 .. 128 bytes: one, two and three SHA-256 blocks with the padding at
    each of its edges.  The item is the batch's first (behind the front pad of the text buffer,
    alignment 0) and its last (in front of the tail, at `align` modulo 16, which is also where
    its span of the message buffer starts)."""
    import hashlib
    for ser_len in (55, 56, 63, 64, 65, 119, 120, 127, 128):
        item, ser = _sized(ser_len)
        filler = b"#" * ((align - len(item)) % 16 + 16)  # (not JSON: the host's)
        texts = [item, filler, item]
        assert (len(item) + len(filler)) % 16 == align
        status, dig, have = _kernel_equals_twin(gpu_engine, hostcheck, texts)
        assert status.tolist() == [0, 1, 0] and have.tolist() == [True, False, True]
        assert dig[0].tobytes() == dig[2].tobytes() == hashlib.sha256(ser).digest()
        assert dig[0].tobytes() == wdd.definition(json.loads(item))


def test_the_longest_text_next_to_one_too_long(gpu_engine, hostcheck):
    head = ('{"identifier":"i","reqId":1,"signature":"%s","operation":{"a":"' % _SIG).encode()
    longest = head + b"x" * (4096 - len(head) - 3) + b'"}}'
    too_long = head + b"x" * (4097 - len(head) - 3) + b'"}}'
    assert (len(longest), len(too_long)) == (4096, 4097)
    for texts in ([longest, too_long], [too_long, longest], [longest]):
        status, dig, have = _kernel_equals_twin(gpu_engine, hostcheck, texts)
        for t, st, h, row in zip(texts, status, have, dig):
            assert (st == 0) == bool(h) == (len(t) == 4096)
            if h:
                assert row.tobytes() == wdd.definition(json.loads(t))
    ser = serialize_msg_for_signing(json.loads(longest), topLevelKeysToIgnore=["signature"])
    assert (len(ser) + 8) // 64 + 1 >= 62  # (SHA-256 blocks)


def test_eligible_ineligible_and_host_items_lane_by_lane(gpu_engine, hostcheck):
    r = random.Random(3)
    texts = []
    for i in range(100):
        d = wire_model.nym_dict(r, i)
        texts.append(wire_model.render(r, d))
        d2 = dict(wire_model.nym_dict(r, i), taaAcceptance={"time": i})
        texts.append(wire_model.render(r, d2))
        d3 = wire_model.nym_dict(r, i)
        d3["operation"]["amount"] = 1.5
        texts.append(wire_model.render(r, d3))
    status, _, have = _kernel_equals_twin(gpu_engine, hostcheck, texts, base=5)
    assert status.tolist() == [0, 0, 1] * 100 and have.tolist() == [True, False, False] * 100


# ------------------------------------------------------------------ call order
@pytest.fixture(scope="module")
def signed(gpu_engine):
    """384 signed NYM requests over 4 GPU-signed keys: (pk, identifiers, verkeys, dicts, flags).
    Every third signature forged; some signers unknown; some requests with another top-level key
    (signed, so accepted, but not eligible); some with a float (the host's grammar, accepted)."""
    from plenum_amd import pack_messages
    from plenum_amd.synth import nym_request, signer_seeds
    n, k = 384, 4
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    vks = ["~" + wire_model.b58(bytes(p[16:])) for p in pk]
    r = random.Random(17)
    kidx = (np.arange(n) % k).astype(np.uint32)
    dicts = []
    for i in range(n):
        d = nym_request("nobody-%d" % (i % 2) if i % 29 == 7 else idrs[i % k], 1_500_000_000_000_000 + i,
                        wire_model.b58(r.randbytes(16)), "~" + wire_model.b58(r.randbytes(16)),
                        alias="a%d" % i if i % 5 == 0 else None)
        if i % 7 == 1:
            d["taaAcceptance"] = {"mechanism": "m", "time": i}
        if i % 13 == 2:
            d["operation"]["amount"] = 1.5
        if i % 31 == 4:
            del d["protocolVersion"]
        dicts.append(d)
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    buf, off = pack_messages(sers)
    sig = gpu_engine.sign_batch(sk, kidx, buf, off)
    sig[::3, 40] ^= 1
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    return pk, idrs, vks, dicts


def test_digests_before_and_after_the_verify(gpu_engine, signed):
    pk, idrs, _, dicts = signed
    plain = [d for d in dicts if d["identifier"] in idrs and "amount" not in d["operation"]]
    r = random.Random(2)
    buf, off = wire_model.pack_texts([wire_model.render(r, d) for d in plain])
    where = {idr: j for j, idr in enumerate(idrs)}
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(pk)

        def verdicts(with_digests):
            status, _ = gpu_engine.wire_scan(buf, off)
            assert not status.any()
            before = gpu_engine.wire_digests() if with_digests else None
            uidx, uniq_item = gpu_engine.wire_idents()
            kid_u = np.array([first + where[plain[i]["identifier"]] for i in uniq_item.tolist()], np.uint32)
            ok = gpu_engine.wire_verify_idents(kid_u)
            after = gpu_engine.wire_digests() if with_digests else None
            return ok, before, after, gpu_engine.wire_verify_idents(kid_u)

        ok, before, after, again = verdicts(True)
        ok_without, _, _, _ = verdicts(False)
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    assert (ok == ok_without).all() and (ok == again).all() and 0 < ok.sum() < len(plain)
    want_have = [wdd.eligible(d) for d in plain]
    assert before[1].tolist() == want_have and any(want_have) and not all(want_have)
    for d, h, row in zip(plain, before[1], before[0]):
        assert row.tobytes() == (wdd.definition(d) if h else bytes(32))
    # into the caller's pinned memory
    pinned = gpu_engine.host_alloc(33 * len(plain) + 64)
    dig_p, have_p = gpu_engine.wire_digests(pinned)
    assert (dig_p == before[0]).all() and (have_p == before[1]).all()
    assert np.frombuffer(pinned, np.uint8, count=32 * len(plain)).tobytes() == before[0].tobytes()


def test_no_wire_batch_is_einval():
    from plenum_amd import EdVerifyEngine
    with EdVerifyEngine(0) as eng:
        with pytest.raises(Exception) as ei:
            eng.wire_digests()
        assert getattr(ei.value, "code", None) == -1, ei.value
        status, _ = eng.wire_scan(*wire_model.pack_texts([]))  # an empty batch is a batch
        dig, have = eng.wire_digests()
        assert len(status) == 0 and dig.shape == (0, 32) and have.shape == (0,)
        eng.wire_scan(*wire_model.pack_texts([wire_model.corpus()[0]]))
        dig, have = eng.wire_digests()
        assert have.tolist() == [True] and dig[0].tobytes() == wdd.definition(json.loads(wire_model.corpus()[0]))


# ------------------------------------------------------------------ through the authenticator
def _authenticator(gpu_engine, idrs, vks, max_keys):
    from plenum_amd.client_authn import GpuAuthNr
    a = GpuAuthNr(engine=gpu_engine, max_keys=max_keys)
    for idr, vk in zip(idrs, vks):
        a.addIdr(idr, vk)
    a.keys_settle()
    return a


def _check_triple(gpu_engine, a, flat, digest, have, dicts):
    """The contract against request_digests over the decoded dicts, and the counters."""
    from plenum_amd.request_digest import request_digests
    n = len(dicts)
    assert len(flat) == n and digest.shape == (n, 32) and have.shape == (n,)
    assert digest.dtype == np.uint8 and have.dtype == bool
    accepted = [not isinstance(x, Exception) for x in flat]
    assert have.tolist() == accepted
    want = request_digests([d for d, ok in zip(dicts, accepted) if ok], gpu_engine)
    assert [digest[i].tobytes().hex() for i in np.flatnonzero(have).tolist()] == want
    assert not digest[~have].any()
    # forged thirds and the unknown signers rejected, everything else accepted
    assert accepted == [i % 3 != 0 and not d["identifier"].startswith("nobody") for i, d in enumerate(dicts)]
    on_host = sum(1 for d, ok in zip(dicts, accepted) if ok and (not wdd.eligible(d) or "amount" in d["operation"]))
    st = a.stats
    assert st["wire_digest_gpu"] > 0 and st["wire_digest_host"] == on_host > 0
    assert st["wire_digest_gpu"] + st["wire_digest_host"] == sum(accepted)


@pytest.mark.parametrize("max_keys", [16, 2])
def test_authenticate_wire_batch_with_digests(gpu_engine, signed, max_keys):
    _, idrs, vks, dicts = signed
    r = random.Random(9)
    texts = [wire_model.render(r, d) for d in dicts]
    with _own_keys(gpu_engine):
        a = _authenticator(gpu_engine, idrs, vks, max_keys)
        results, digest, have = a.authenticate_wire_batch(texts, digests=True)
        _check_triple(gpu_engine, a, results, digest, have, dicts)
        if max_keys == 2:  # two slots for four keys: the general path is taken
            assert a.stats["keyed_items"] < a.stats["batch_items"]
        b = _authenticator(gpu_engine, idrs, vks, max_keys)
        plain = b.authenticate_wire_batch(texts)
        assert type(plain) is list and [type(x) for x in plain] == [type(x) for x in results]
        assert b.stats["wire_digest_gpu"] == b.stats["wire_digest_host"] == 0


@pytest.mark.parametrize("split", ["1", "0"])
def test_authenticate_node_wire_batch_with_digests(gpu_engine, signed, monkeypatch, split):
    from plenum_amd.nodeloop import batch_text, propagate_text
    _, idrs, vks, dicts = signed
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(dicts)]
    prepare = json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 9, "digest": "d", "txnRootHash": None})
    entries = [batch_text(props[k:k + 40] + [prepare] + props[k + 40:k + 96]).encode() for k in range(0, 384, 96)]
    monkeypatch.setenv("EDV_WIRE_SPLIT", split)  # (read when the authenticator is made)
    with _own_keys(gpu_engine):
        a = _authenticator(gpu_engine, idrs, vks, 16)
        assert a._g.wire_split_gpu == (split == "1")
        out, digest, have = a.authenticate_node_wire_batch(entries, digests=True)
        assert [len(o) for o in out] == [96] * 4
        _check_triple(gpu_engine, a, [x for o in out for x in o], digest, have, dicts)
        b = _authenticator(gpu_engine, idrs, vks, 16)
        plain = b.authenticate_node_wire_batch(entries)
        assert type(plain) is list and [len(o) for o in plain] == [96] * 4
