"""The node wire path on the MI355X: edv_wire_unwrap_kernel + the unchanged scan against their
CPU twins (hc_wire_unwrap, then hc_wire_scan over the twin's unwrapped buffer), byte for byte
through edv_wire_readback; edv_wire_ident_text against slices of the twin's buffer; and
authenticate_node_wire_batch against the host definition and the C oracle on a GpuAuthNr."""
import contextlib
import json
import random

import numpy as np
import pytest

import wire_model
import wire_unwrap_model as wum
from engine_double import OracleEngine

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def node_messages():
    """Every message of the unwrap corpus as the splitter cuts it, plus every entry whole
    (a BATCH the splitter would have cut, as one the GPU must leave to the host) and the scan
    corpus's bare request texts: [(body, esc)]."""
    corp = wum.corpus()
    entries = corp["clean"] + corp["mutated"]
    return (wum.messages(entries) + [(e, 0) for e in entries] + [(e, 1) for e in corp["mutated"][::5]]
            + [(t, 0) for t in wire_model.corpus()[::9]])


def _pack(msgs, base):
    buf, off = wire_model.pack_texts([b for b, _ in msgs], base=base)
    return buf, off, np.array([e for _, e in msgs], np.uint8)


def _check_against_twins(eng, hostcheck, msgs, base):
    buf, off, esc = _pack(msgs, base)
    cls, status, span = eng.wire_scan_node(buf, off, esc)
    sig, out, mlen = eng.wire_readback()
    t_cls, t_text = wum.twin_unwrap(hostcheck, buf[base:], off - off[0], esc)
    t_status, t_span, t_sig, t_out, t_mlen = wire_model.twin_scan(hostcheck, t_text, off - off[0])
    assert cls.tolist() == t_cls.tolist()
    assert status.tolist() == t_status.tolist()
    assert span.tolist() == t_span.tolist()
    assert mlen.tolist() == t_mlen.tolist()
    assert not status[cls != 0].tolist().count(0)  # only a request is ever scanned
    ok = np.flatnonzero(status == 0)
    assert (sig[ok] == t_sig[ok]).all()
    for i in ok.tolist():
        a = int(off[i] - off[0])
        assert out[a:a + int(mlen[i])].tobytes() == t_out[a:a + int(t_mlen[i])].tobytes(), (i, msgs[i])
    return cls, status, span, t_text


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096])
def test_unwrap_and_scan_equal_their_cpu_twins(gpu_engine, hostcheck, node_messages, n):
    """Shuffled corpus messages: lanes without an item, a workgroup boundary, 10-byte and 4 KiB
    neighbours in one LDS tile, messages straddling tile boundaries, over-long ones between
    scanned ones."""
    r = random.Random(200 + n)
    cls, status, _, _ = _check_against_twins(gpu_engine, hostcheck, r.choices(node_messages, k=n), 0)
    if n == 4096:
        assert (cls == 0).sum() >= 1000 and (cls == 1).sum() >= 1000 and (cls == 2).sum() >= 100
        assert (status == 0).sum() >= 1000


def test_an_odd_base_offset_and_a_second_batch(gpu_engine, hostcheck, node_messages):
    r = random.Random(6)
    _check_against_twins(gpu_engine, hostcheck, r.choices(node_messages, k=777), 7)
    second = r.choices(node_messages, k=130)  # a second call replaces the batch
    _check_against_twins(gpu_engine, hostcheck, second, 1)
    sig, out, mlen = gpu_engine.wire_readback()
    assert sig.shape == (130, 64) and len(mlen) == 130 and len(out) == sum(len(b) for b, _ in second)
    with pytest.raises(Exception) as ei:
        gpu_engine.wire_verify(np.full(777, 0xFFFFFFFE, np.uint32))  # the first batch's item count
    assert getattr(ei.value, "code", None) == -1
    # a plain scan after it is the plain scan (the node call leaves nothing behind)
    texts = [b for b, e in second if not e]
    buf, off = wire_model.pack_texts(texts)
    status, span = gpu_engine.wire_scan(buf, off)
    t = wire_model.twin_scan(hostcheck, buf, off)
    assert status.tolist() == t[0].tolist() and span.tolist() == t[1].tolist()


def test_wire_ident_text(gpu_engine, hostcheck):
    """5 identifiers over 300 items; one's first occurrence sits in an escaped message."""
    from plenum_amd.nodeloop import batch_text, propagate_text
    r = random.Random(4)
    idrs = ["idr-%d-%s" % (k, "x" * (3 * k)) for k in range(5)]
    reqs = []
    for i in range(300):
        d = wire_model.nym_dict(r, i)
        d["identifier"] = idrs[(i * 7) % 5 if i >= 5 else [2, 0, 4, 1, 3][i]]
        reqs.append(d)
    entries = [json.dumps(reqs[0]).encode(), propagate_text(reqs[1], "c").encode()]
    entries += [batch_text([propagate_text(d, 'c"%d' % i) for i, d in enumerate(reqs[k:k + 50], k)]).encode()
                for k in (2, 52, 102, 152, 202, 252)]
    entries[-1] = entries[-1][:-1] + b" }"
    msgs = wum.messages(entries)[:300]
    assert len(msgs) == 300 and [e for _, e in msgs[:3]] == [0, 0, 1]
    _, status, span, t_text = _check_against_twins(gpu_engine, hostcheck, msgs, 3)
    assert not status.any()
    uidx, uniq_item = gpu_engine.wire_idents()
    assert uniq_item.tolist() == [0, 1, 2, 3, 4]  # identifier 4 first in an escaped message (item 2)
    got = gpu_engine.wire_ident_text(uniq_item)
    off = np.cumsum([0] + [len(b) for b, _ in msgs])
    want = [t_text[int(off[i]) + int(span[i, 0]):int(off[i]) + int(span[i, 0]) + int(span[i, 1])].tobytes()
            for i in uniq_item.tolist()]
    assert got == want == [idrs[k].encode() for k in (2, 0, 4, 1, 3)]
    assert gpu_engine.wire_ident_text(uniq_item[[3, 3, 0]]) == [want[3], want[3], want[0]]
    assert gpu_engine.wire_ident_text(uniq_item[:0]) == []
    assert [idrs.index(s.decode()) for s in gpu_engine.wire_ident_text(np.arange(300, dtype=np.uint32))] == \
        [[2, 0, 4, 1, 3][i] if i < 5 else (i * 7) % 5 for i in range(300)]


@pytest.fixture(scope="module")
def node_drain(gpu_engine):
    """3 client requests, 2 bare PROPAGATEs and 3 BATCHes of 70 members over 8 GPU-signed keys,
    every third S corrupted; one unknown identifier, one whose getVerkey raises, one member with
    a \\u escape (the host decodes it), PREPARE-like members, one undecodable entry.
    (pk, identifiers, verkeys, entries, per request in drain order: (key index, sig64, ser))."""
    from plenum_amd import pack_messages
    from plenum_amd.nodeloop import batch_text, propagate_text
    from plenum_amd.serialization import serialize_msg_for_signing
    from plenum_amd.synth import nym_request, signer_seeds
    k = 8
    n = 3 + 2 + 3 * 68
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    vks = ["~" + wire_model.b58(bytes(p[16:])) for p in pk]
    r = random.Random(31)
    kidx = (np.arange(n) % k).astype(np.uint32)
    names = list(idrs)
    dicts = []
    for i in range(n):
        idr = {20: "nobody", 33: "boom-1"}.get(i, names[i % k])
        dicts.append(nym_request(idr, 1_500_000_000_000_000 + i, wire_model.b58(r.randbytes(16)),
                                 "~" + wire_model.b58(r.randbytes(16)), alias="a%d" % i if i % 5 == 0 else None))
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    buf, off = pack_messages(sers)
    sig = gpu_engine.sign_batch(sk, kidx, buf, off)
    sig[::3, 40] ^= 1
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    prepare = json.dumps({"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 9, "digest": "d", "txnRootHash": None})
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(dicts)]
    props[50] = props[50].replace("client50", "client\\u0035\\u0030")  # the same message, host-decoded
    entries = [json.dumps(d) for d in dicts[:3]] + props[3:5]
    for b in range(3):
        members = props[5 + 68 * b:5 + 68 * (b + 1)]
        entries.append(batch_text(members[:30] + [prepare] + members[30:] + [prepare]))
    entries.insert(4, '{"op": "PROPAGATE", "request": {"signature": ')  # undecodable
    assert [len(json.loads(e)["messages"]) for e in entries[-3:]] == [70, 70, 70]
    return pk, idrs, vks, [e.encode() for e in entries], kidx, sig, sers


class _Boom(Exception):
    pass


@pytest.mark.parametrize("max_keys", [16, 2])
def test_authenticate_node_wire_batch_end_to_end(gpu_engine, oracle, node_drain, max_keys):
    from plenum_amd import pack_messages
    from plenum_amd.batching import requests_in_drain
    from plenum_amd.client_authn import GpuAuthNr
    pk, idrs, vks, entries, kidx, sig, sers = node_drain

    class Raising(GpuAuthNr):
        def getVerkey(self, identifier):
            if identifier.startswith("boom"):
                raise _Boom(identifier)
            return super().getVerkey(identifier)

    with _own_keys(gpu_engine):
        wire, plain = (Raising(engine=gpu_engine, max_keys=max_keys) for _ in range(2))
        for a in (wire, plain):
            for idr, vk in zip(idrs, vks):
                a.addIdr(idr, vk)
            a.keys_settle()
        got = wire.authenticate_node_wire_batch(entries)
        want = plain.authenticate_batch(requests_in_drain(entries))
    assert [len(g) for g in got] == [len(requests_in_drain([e])) for e in entries]
    assert [len(g) for g in got] == [1, 1, 1, 1, 0, 1, 68, 68, 68]
    flat = [x for g in got for x in g]
    assert len(flat) == len(want) == len(sers)
    for i, (g, w) in enumerate(zip(flat, want)):
        assert type(g) is type(w), (i, g, w)
        if isinstance(w, Exception):
            assert g.args == w.args and type(g.__cause__) is type(w.__cause__), (i, g, w)
        else:
            assert g == w
    # the accepted set is the C oracle's crypto_sign_open on sig || ser
    buf, off = pack_messages(sers)
    expect = OracleEngine(oracle).verify_batch(sig, pk[kidx], buf, off)
    expect[[20, 33]] = False  # the unknown identifier; the one whose getVerkey raises
    assert [isinstance(g, str) for g in flat] == expect.tolist()
    assert expect.sum() >= 130
    assert isinstance(flat[20], Exception) and isinstance(flat[33], Exception)
    # the messages the host decoded: the \u member and the undecodable entry
    msgs = wum.messages(entries)
    cls = [wum.unwrap(b, e)[0] for b, e in msgs]
    assert cls.count(wum.HOST) == 2 and cls.count(wum.NONE) == 6
    st = wire.stats
    assert st["wire_host_items"] == cls.count(wum.HOST)
    assert st["wire_items"] == len(msgs) - 8 == len(sers) - 1
    if max_keys == 16:  # every key registered: the keyed path alone
        assert st["keyed_items"] == st["batch_items"] > 0
    else:  # two slots for eight keys: the general path is taken
        assert st["keyed_items"] < st["batch_items"]
