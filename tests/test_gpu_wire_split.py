"""The BATCH split on the MI355X: edv_wire_scan_entries (edv_node_split_count_kernel,
edv_node_split_emit_kernel, edv_node_copy_kernel, then the unchanged unwrap and scan) against the
host split (_hostpack.gather_node_texts) byte for byte, and against edv_wire_scan_node over the
host-gathered form of the same entries; then authenticate_node_wire_batch on a GpuAuthNr with the
GPU split and with the host split."""
import json
import random

import numpy as np
import pytest

import node_split_cases as nsc
import wire_model
import wire_unwrap_model as wum
from engine_double import OracleEngine
from test_gpu_wire_node import _Boom, _own_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    return nsc.corpus_entries() + nsc.count_entries() + nsc.sweep_entries()[::9]


def _check(eng, entries, base=0):
    """wire_scan_entries over the entries against the host split and wire_scan_node."""
    text, eoff = nsc.pack(entries, base)
    cls, status, span, esc, entry, at, off = eng.wire_scan_entries(text, eoff)
    raw = eng.wire_raw_readback()
    sig, msgs, mlen = eng.wire_readback()
    h_off, h_esc, h_entry, h_bodies = nsc.host_split(entries)
    assert off.tolist() == h_off.tolist()
    assert esc.tolist() == h_esc.tolist()
    assert entry.tolist() == h_entry.tolist()
    assert raw.tobytes() == h_bodies.tobytes()
    assert nsc.bodies_at(text, off, at).tobytes() == h_bodies.tobytes()
    n_cls, n_status, n_span = eng.wire_scan_node(h_bodies, h_off, h_esc)
    n_sig, n_msgs, n_mlen = eng.wire_readback()
    assert cls.tolist() == n_cls.tolist()
    assert status.tolist() == n_status.tolist()
    assert span.tolist() == n_span.tolist()
    assert mlen.tolist() == n_mlen.tolist()
    ok = np.flatnonzero(status == 0)
    assert (sig[ok] == n_sig[ok]).all()
    for i in ok.tolist():
        a = int(off[i])
        assert msgs[a:a + int(mlen[i])].tobytes() == n_msgs[a:a + int(mlen[i])].tobytes(), i
    return cls, status, esc, entry


@pytest.mark.parametrize("n_e", [0, 1, 63, 64, 65, 1000])
def test_entries_equal_the_host_split_and_the_node_scan(gpu_engine, pool, n_e):
    """Shuffled entries: waves without an entry, a workgroup boundary, BATCHes of 130 members
    between 10-byte entries, every alignment of an entry in its 16 bytes."""
    r = random.Random(300 + n_e)
    cls, status, esc, entry = _check(gpu_engine, r.choices(pool, k=n_e), base=n_e % 7)
    if n_e == 1000:
        assert len(set(entry[esc == 1].tolist())) >= 100 and (esc == 0).sum() >= 300
        assert (status == 0).sum() >= 100 and (cls == 2).sum() >= 50


def test_the_boundary_sweep_in_one_call(gpu_engine):
    sweep = nsc.sweep_entries()
    _, _, esc, entry = _check(gpu_engine, sweep)
    assert len(esc) == len(sweep) and esc.sum() >= 1000 and (esc == 0).sum() >= 1000


def test_member_counts_and_whole_corpus(gpu_engine):
    entries = nsc.corpus_entries() + nsc.count_entries()
    _, _, esc, entry = _check(gpu_engine, entries, base=3)
    members = np.bincount(entry[esc == 1], minlength=len(entries)).tolist()
    assert {1, 2, 63, 64, 65, 70, 130} <= set(members)


def test_a_second_call_replaces_the_batch_and_a_plain_scan_follows(gpu_engine, hostcheck, pool):
    r = random.Random(8)
    _check(gpu_engine, r.choices(pool, k=300))
    second = r.choices(pool, k=40)
    text, eoff = nsc.pack(second, 1)
    out = gpu_engine.wire_scan_entries(text, eoff)
    h_off, h_esc, _, h_bodies = nsc.host_split(second)
    assert out[6].tolist() == h_off.tolist() and gpu_engine.wire_raw_readback().tobytes() == h_bodies.tobytes()
    sig, msgs, mlen = gpu_engine.wire_readback()
    assert sig.shape == (len(h_esc), 64) and len(msgs) == int(h_off[-1])
    with pytest.raises(Exception) as ei:
        gpu_engine.wire_verify(np.full(len(h_esc) + 1, 0xFFFFFFFE, np.uint32))  # not this batch's item count
    assert getattr(ei.value, "code", None) == -1
    # nothing but empty BATCHes: an empty batch
    empty = gpu_engine.wire_scan_entries(*nsc.pack([nsc.batch_of([])] * 5))
    assert [len(x) for x in empty] == [0, 0, 0, 0, 0, 0, 1] and len(gpu_engine.wire_raw_readback()) == 0
    # descending offsets are refused
    with pytest.raises(Exception) as ei:
        gpu_engine.wire_scan_entries(text, np.array([5, 3, 9], np.uint64))
    assert getattr(ei.value, "code", None) == -1
    # a plain scan afterwards is the plain scan, and its batch is no batch of entries
    texts = [e for e in second if nsc.host_split([e])[1].tolist() == [0]]
    buf, off = wire_model.pack_texts(texts)
    status, span = gpu_engine.wire_scan(buf, off)
    t = wire_model.twin_scan(hostcheck, buf, off)
    assert status.tolist() == t[0].tolist() and span.tolist() == t[1].tolist()
    with pytest.raises(Exception) as ei:
        gpu_engine.wire_raw_readback()
    assert getattr(ei.value, "code", None) == -1


def test_idents_after_entries_equal_those_after_the_node_scan(gpu_engine):
    entries = wum.corpus()["clean"] * 3
    random.Random(2).shuffle(entries)
    text, eoff = nsc.pack(entries)
    _, status, span, esc, _, _, off = gpu_engine.wire_scan_entries(text, eoff)
    uidx, uniq_item = gpu_engine.wire_idents()
    idents = gpu_engine.wire_ident_text(uniq_item)
    h_off, h_esc, _, h_bodies = nsc.host_split(entries)
    _, n_status, n_span = gpu_engine.wire_scan_node(h_bodies, h_off, h_esc)
    n_uidx, n_uniq_item = gpu_engine.wire_idents()
    assert status.tolist() == n_status.tolist() and (status == 0).sum() >= 100 and esc.sum() >= 100
    assert uidx.tolist() == n_uidx.tolist() and uniq_item.tolist() == n_uniq_item.tolist()
    assert idents == gpu_engine.wire_ident_text(n_uniq_item) and len(idents) >= 20


@pytest.fixture(scope="module")
def node_drain(gpu_engine):
    """test_gpu_wire_node's drain again: 3 client requests, 2 bare PROPAGATEs and 3 BATCHes of 70
    members over 8 GPU-signed keys, every third S corrupted; one unknown identifier, one whose
    getVerkey raises, one member with a \\u escape (the host decodes it), PREPARE-like members, one
    undecodable entry.  (pk, identifiers, verkeys, entries, key index, sig64, ser per request.)"""
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
    dicts = []
    for i in range(n):
        idr = {20: "nobody", 33: "boom-1"}.get(i, idrs[i % k])
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
    return pk, idrs, vks, [e.encode() for e in entries], kidx, sig, sers


def test_authenticate_node_wire_batch_on_both_splits(gpu_engine, oracle, node_drain):
    from plenum_amd import pack_messages
    from plenum_amd.client_authn import GpuAuthNr
    pk, idrs, vks, entries, kidx, sig, sers = node_drain
    assert gpu_engine.supports_wire_split

    class Raising(GpuAuthNr):
        def getVerkey(self, identifier):
            if identifier.startswith("boom"):
                raise _Boom(identifier)
            return super().getVerkey(identifier)

    ran = []
    for split_gpu in (True, False):  # (each with the engine's key store to itself: the same counters)
        with _own_keys(gpu_engine):
            a = Raising(engine=gpu_engine, max_keys=16)
            a._g.wire_split_gpu = split_gpu
            for idr, vk in zip(idrs, vks):
                a.addIdr(idr, vk)
            a.keys_settle()
            ran.append((a, a.authenticate_node_wire_batch(entries)))
    (gpu, got), (host, other) = ran
    assert [len(g) for g in got] == [len(g) for g in other] == [1, 1, 1, 1, 0, 1, 68, 68, 68]
    flat, flat_other = [x for g in got for x in g], [x for g in other for x in g]
    assert len(flat) == len(flat_other) == len(sers)
    for i, (g, w) in enumerate(zip(flat, flat_other)):
        assert type(g) is type(w), (i, g, w)
        if isinstance(w, Exception):
            assert g.args == w.args and type(g.__cause__) is type(w.__cause__), (i, g, w)
        else:
            assert g == w
    assert gpu.stats == host.stats
    assert gpu.stats["wire_host_items"] == 2 and gpu.stats["wire_items"] == len(sers) - 1
    assert gpu.stats["keyed_items"] == gpu.stats["batch_items"] > 0
    # the accepted set is the C oracle's crypto_sign_open on sig || ser
    buf, off = pack_messages(sers)
    expect = OracleEngine(oracle).verify_batch(sig, pk[kidx], buf, off)
    expect[[20, 33]] = False  # the unknown identifier; the one whose getVerkey raises
    assert [isinstance(g, str) for g in flat] == expect.tolist()
    assert [isinstance(g, str) for g in flat_other] == expect.tolist()
    assert expect.sum() >= 130
