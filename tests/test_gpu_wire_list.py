"""edv_wire_verify_list on the MI355X: the GPU-built work list (edv_wire_once_*_kernel,
csrc/wire_once.h) in front of the unchanged verify kernels against edv_wire_verify over the
same per-item keys and against the C oracle, with and without verifying each distinct request
once; its lane count against the CPU twin and a Python dict; its preconditions; and
authenticate_node_wire_batch over a mixed drain for the four switch settings."""
import contextlib
import json
import random

import numpy as np
import pytest

import wire_model
from engine_double import OracleEngine
from test_wire_once import adversarial_texts
from wire_list_double import DEAD, DEVICE_PROBE, NO_ID, SKIP, device_cap, dict_oracle, mixed_drain, twin_once

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 129, 4160]
PREPARE = b'{"op": "PREPARE", "instId": 0, "viewNo": 0, "ppSeqNo": 9, "ppTime": 1500000000, "digest": "d"}'


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
def pool(gpu_engine, oracle):
    """400 NYM requests over 8 GPU-signed keys (signers 0 - 3 to be registered, 4 - 5 verified
    from their key bytes, 6 skipped, 7 only ever in texts the host decides), every third S
    corrupted; request 1 a forged signature (zeros), request 2 request 4's valid signature over
    a request that differs in one digit.  (pk, identifiers, texts, signer per request, the
    C oracle's verdict per request.)"""
    from plenum_amd import pack_messages
    from plenum_amd.serialization import serialize_msg_for_signing
    from plenum_amd.synth import nym_request, signer_seeds
    n, k = 400, 8
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    r = random.Random(41)
    kidx = (np.arange(n) % k).astype(np.uint32)
    kidx[[1, 2, 4]] = 0
    dicts = [nym_request(idrs[kidx[i]], 1_500_000_000_000_000 + i, wire_model.b58(r.randbytes(16)),
                         "~" + wire_model.b58(r.randbytes(16)), alias="a%d" % i if i % 5 == 0 else None)
             for i in range(n)]
    dicts[2] = dict(dicts[4], reqId=dicts[4]["reqId"] + 1)  # (the same length: the last digit differs)
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    assert len(sers[2]) == len(sers[4]) and sers[2] != sers[4]
    buf, off = pack_messages(sers)
    sig = gpu_engine.sign_batch(sk, kidx, buf, off)
    sig[::3, 40] ^= 1
    sig[1] = 0
    sig[2] = sig[4]
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    texts = [json.dumps(d).encode() for d in dicts]
    want = OracleEngine(oracle).verify_batch(sig, pk[kidx], buf, off)
    assert want[4] and not want[1] and not want[2] and 200 < want.sum() < 300
    return pk, idrs, texts, kidx, want


def _dead_positions(n):
    """Dead items in every lane position class: lane 0, lane 63, a whole wave, the last
    (partial) wave's last item, and a sprinkle."""
    dead = set()
    if n >= 63:
        dead |= {0, 62 if n == 63 else 63}
    if n >= 65:
        dead.add(n - 1)
    if n >= 129:
        dead.add(64)
    if n >= 4160:
        dead |= set(range(128, 192)) | set(range(200, n, 37))
    return dead


def _batch(pool, n, seed):
    """n messages: (texts, the pool request of each or -1, expected verdicts)."""
    pk, idrs, texts, kidx, want = pool
    r = random.Random(seed)
    dead = _dead_positions(n)
    usable = [q for q in range(len(texts)) if kidx[q] != 7]
    draw = []
    if n - len(dead) >= 60:
        draw += [1] * 24 + [4] * 24 + [2] * 2  # the forged signature and a valid one 24 times each
    while len(draw) < n - len(dead):
        draw += [r.choice(usable)] * r.choice([1, 1, 1, 2, 2, 24])
    draw = draw[:n - len(dead)]
    r.shuffle(draw)
    over_long = [q for q in range(len(texts)) if kidx[q] == 7]
    out, req = [], []
    for i in range(n):
        if i in dead:
            kind = r.randrange(3)
            if kind == 0:
                out.append(PREPARE)  # no signed request inside
            elif kind == 1:  # a request of the identifier no scanned item has, too long for the GPU
                t = texts[r.choice(over_long)]
                out.append(t[:-1] + b" " * (wire_model.MAX_TEXT + 1 - len(t)) + b"}")
            else:
                out.append(texts[r.choice(usable)][:-1] + b', "x": 1.5}')  # a float: the host decides
            req.append(-1)
        else:
            q = draw.pop()
            out.append(b" " * r.randrange(4) + texts[q])  # (a copy at another alignment)
            req.append(q)
    req = np.array(req, np.int64)
    expect = np.where(req >= 0, want[np.maximum(req, 0)] & (kidx[np.maximum(req, 0)] != 6), False)
    return out, req, expect


def _keys_per_identifier(eng, pool, first, uniq_item):
    pk, idrs, _, _, _ = pool
    names = [b.decode("ascii") for b in eng.wire_ident_text(uniq_item)]
    nu = len(names)
    kid_u = np.full(nu, SKIP, np.uint32)
    pk_u = np.zeros((nu, 32), np.uint8)
    for j, name in enumerate(names):
        s = idrs.index(name)
        assert s != 7
        if s < 4:
            kid_u[j] = first + s
        elif s < 6:
            kid_u[j] = NO_ID
            pk_u[j] = pk[s]
    return kid_u, pk_u


@pytest.mark.parametrize("n", SIZES)
def test_the_list_equals_wire_verify_and_the_oracle(gpu_engine, hostcheck, pool, n):
    texts, req, expect = _batch(pool, n, 500 + n)
    buf, off = wire_model.pack_texts(texts, base=3)
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(pool[0][:4])
        cls, status, _ = gpu_engine.wire_scan_node(buf, off, np.zeros(n, np.uint8))
        assert (status != 0).tolist() == (req < 0).tolist()
        uidx, uniq_item = gpu_engine.wire_idents()
        nu = len(uniq_item)
        kid_u, pk_u = _keys_per_identifier(gpu_engine, pool, first, uniq_item)
        if n >= 4160:
            assert nu == 7 and (kid_u == NO_ID).sum() == 2 and (kid_u == SKIP).sum() == 1
            assert (cls == gpu_engine.NODE_NONE).sum() > 10 and (status[cls != gpu_engine.NODE_NONE] != 0).sum() > 10
        key_id = np.append(kid_u, np.uint32(SKIP))[uidx]
        pk32 = np.concatenate([pk_u, np.zeros((1, 32), np.uint8)])[uidx]
        plain = gpu_engine.wire_verify(key_id, pk32) if n else np.zeros(0, bool)
        assert plain.tolist() == expect.tolist()
        sig, msgs, mlen = gpu_engine.wire_readback()
        start = (off[:-1] - off[0]).astype(np.uint64)
        args = (sig, msgs, start, start + mlen, status, uidx, kid_u)
        want_rep, want_grp = dict_oracle(*args)
        live = sum(1 for g in want_grp if g != DEAD)
        distinct = sum(1 for i in range(n) if want_grp[i] != DEAD and want_rep[i] == i)
        # the precondition that makes the lane count exact in any arrival order
        lanes, rep, _, gave, run = twin_once(hostcheck, *args)
        assert run < DEVICE_PROBE and gave == 0 and lanes == distinct and rep.tolist() == want_rep
        for once in (False, True):
            ok, m = gpu_engine.wire_verify_list(kid_u, pk_u, once)
            assert ok.tolist() == plain.tolist(), once
            assert m == (distinct if once else live)
        if n >= 4160:
            assert distinct < live // 2 and live > 3000
        # without general identifiers pk_u may be absent
        keyed_only = np.where(kid_u == NO_ID, np.uint32(SKIP), kid_u)
        ok, m = gpu_engine.wire_verify_list(keyed_only, None, True)
        assert ok.tolist() == (plain & (key_id != NO_ID)).tolist()


def test_the_adversarial_batch(gpu_engine, oracle, hostcheck):
    """200 items of one identifier and ONE signature over pairwise different requests of one
    length: one home slot, a chain the device bound cuts at 128 -- the rest stand for themselves."""
    from test_wire_authn import _Signer
    signer = _Signer(oracle, 1)
    texts = adversarial_texts(signer)
    buf, off = wire_model.pack_texts(texts)
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(np.frombuffer(signer.pk.raw, np.uint8).reshape(1, 32))
        status, _ = gpu_engine.wire_scan(buf, off)
        assert not status.any()
        uidx, uniq_item = gpu_engine.wire_idents()
        assert len(uniq_item) == 1
        kid_u = np.array([first], np.uint32)
        sig, msgs, mlen = gpu_engine.wire_readback()
        assert len(set(mlen.tolist())) == 1 and len({bytes(s) for s in sig}) == 1
        assert device_cap(200) >= 2 * 200
        ok, m = gpu_engine.wire_verify_list(kid_u, None, True)
        assert ok.tolist() == [True] + [False] * 199 == gpu_engine.wire_verify(np.full(200, first, np.uint32)).tolist()
        live = distinct = 200
        assert live >= m >= distinct


def test_preconditions(pool):
    """Every misuse is EDV_EINVAL (-1) and leaves the context usable."""
    from plenum_amd import EdVerifyEngine
    texts, req, expect = _batch(pool, 129, 9)

    def refused(call):
        with pytest.raises(Exception) as ei:
            call()
        assert getattr(ei.value, "code", None) == -1, ei.value

    buf, off = wire_model.pack_texts(texts)
    esc = np.zeros(129, np.uint8)
    with EdVerifyEngine(0) as eng:
        refused(lambda: eng.wire_verify_list(np.zeros(0, np.uint32)))            # a fresh context
        first = eng.keys_add(pool[0][:4])
        eng.wire_scan_node(buf, off, esc)
        refused(lambda: eng.wire_verify_list(np.full(6, first, np.uint32)))      # before wire_idents
        uidx, uniq_item = eng.wire_idents()
        kid_u, pk_u = _keys_per_identifier(eng, pool, first, uniq_item)
        assert (kid_u == NO_ID).any()
        eng.wire_scan_node(buf, off, esc)
        refused(lambda: eng.wire_verify_list(kid_u, pk_u))                       # the batch was rescanned since
        eng.wire_idents()
        refused(lambda: eng.wire_verify_list(kid_u[:-1], pk_u[:-1]))             # a wrong n_uniq
        refused(lambda: eng.wire_verify_list(np.append(kid_u, kid_u[:1]), np.concatenate([pk_u, pk_u[:1]])))
        refused(lambda: eng.wire_verify_list(kid_u, None))                       # NO_ID without pk_u
        ok, m = eng.wire_verify_list(kid_u, pk_u, True)
        assert ok.tolist() == expect.tolist() and 0 < m <= 129
        # uidx survives a list call: the steady call over the all-live prefix of another batch
        live = [t for t, q in zip(texts, req) if q >= 0 and pool[3][q] < 4]
        eng.wire_scan_node(*wire_model.pack_texts(live), np.zeros(len(live), np.uint8))
        uidx2, uniq2 = eng.wire_idents()
        kid2, _ = _keys_per_identifier(eng, pool, first, uniq2)
        a, _ = eng.wire_verify_list(kid2, None, True)
        b = eng.wire_verify_idents(kid2)
        c, _ = eng.wire_verify_list(kid2, None, False)
        assert a.tolist() == b.tolist() == c.tolist() and b.any()
        eng.wire_scan(*wire_model.pack_texts([]))
        eng.wire_idents()
        ok, m = eng.wire_verify_list(np.zeros(0, np.uint32))
        assert len(ok) == 0 and m == 0


class _Boom(Exception):
    pass


@pytest.fixture(scope="module")
def drain(gpu_engine):
    """The mixed drain (wire_list_double.mixed_drain) over 213 requests of 8 GPU-signed keys,
    every third S corrupted; request 30's identifier is unknown, request 41's getVerkey raises.
    (pk, identifiers, verkeys, entries, signer and signature per request, sers)."""
    from plenum_amd import pack_messages
    from plenum_amd.serialization import serialize_msg_for_signing
    from plenum_amd.synth import nym_request, signer_seeds
    k, n = 8, 213
    pk, sk = gpu_engine.seed_keypair_batch(signer_seeds(k))
    idrs = [wire_model.b58(bytes(p[:16])) for p in pk]
    vks = ["~" + wire_model.b58(bytes(p[16:])) for p in pk]
    r = random.Random(32)
    kidx = (np.arange(n) % k).astype(np.uint32)
    dicts = []
    for i in range(n):
        idr = {30: "nobody", 41: "boom-1"}.get(i, idrs[i % k])
        dicts.append(nym_request(idr, 1_500_000_000_000_000 + i, wire_model.b58(r.randbytes(16)),
                                 "~" + wire_model.b58(r.randbytes(16)), alias="a%d" % i if i % 5 == 0 else None))
    sers = [serialize_msg_for_signing(d, topLevelKeysToIgnore=["signature"]) for d in dicts]
    sig = gpu_engine.sign_batch(sk, kidx, *pack_messages(sers))
    sig[::3, 40] ^= 1
    for d, s in zip(dicts, sig):
        d["signature"] = wire_model.b58(bytes(s))
    return pk, idrs, vks, mixed_drain(dicts), kidx, sig, sers


@pytest.mark.parametrize("max_keys", [16, 2])
def test_authenticate_node_wire_batch_end_to_end(gpu_engine, oracle, drain, max_keys):
    from plenum_amd import pack_messages
    from plenum_amd.client_authn import GpuAuthNr
    pk, idrs, vks, entries, kidx, sig, sers = drain

    class Raising(GpuAuthNr):
        def getVerkey(self, identifier):
            if identifier.startswith("boom"):
                raise _Boom(identifier)
            return super().getVerkey(identifier)

    expect = OracleEngine(oracle).verify_batch(sig, pk[kidx], *pack_messages(sers))
    expect[[30, 41]] = False
    existing = ("batches", "batch_items", "keyed_items", "wire_items", "wire_host_items")
    stats = {}
    with _own_keys(gpu_engine):
        for use_list, once in ((False, False), (True, False), (False, True), (True, True)):
            gpu_engine.__dict__.pop("_edv_key_store", None)
            gpu_engine.keys_reset()
            a, plain = (Raising(engine=gpu_engine, max_keys=max_keys) for _ in range(2))
            a._g.wire_list, a._g.wire_once = use_list or once, once
            for x in (a, plain):
                for idr, vk in zip(idrs, vks):
                    x.addIdr(idr, vk)
                x.keys_settle()
            got = a.authenticate_node_wire_batch(entries)
            want = plain._node_wire_decoded(entries)
            assert [len(g) for g in got] == [len(w) for w in want]
            for g, w in zip([x for g in got for x in g], [x for w in want for x in w]):
                assert type(g) is type(w), (use_list, once, g, w)
                if isinstance(w, Exception):
                    assert g.args == w.args and type(g.__cause__) is type(w.__cause__)
                else:
                    assert g == w
            # the accepted set is the C oracle's: the 3 client texts, then every node's PROPAGATEs
            flat = [isinstance(x, str) for g in got for x in g]
            assert len(flat) == 3 + 3 * 210 and flat[:3] == expect[:3].tolist()
            for node in range(3):
                assert flat[3 + 210 * node:3 + 210 * (node + 1)] == expect[3:].tolist()
            stats[(use_list, once)] = dict(a.stats)
    base = stats[(False, False)]
    assert base["wire_list_batches"] == 0 and base["wire_host_items"] == 1 and base["batch_items"] > 600
    for key, st in stats.items():
        assert {k: st[k] for k in existing} == {k: base[k] for k in existing}, key
        if key != (False, False):
            assert st["wire_list_batches"] == 1
    # once: the three nodes' copies are verified once -- about one third of the batch's items
    live = st_once = stats[(True, True)]["wire_distinct_items"]
    assert stats[(True, False)]["wire_distinct_items"] == base["batch_items"] - 1  # (- the \u member, host-verified)
    assert st_once == 213 - 2 and 0.30 < live / base["batch_items"] < 0.37
