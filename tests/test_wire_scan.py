"""The wire scanner on the CPU: the grammar's Python restatement (wire_model.scan) against
json.loads + plenum_amd.serialization, the scanner itself (csrc/wire_scan.h compiled into
libedv_hostcheck.so with every access asserted in bounds) against the restatement, the
reference serializer's KATs, and _hostpack.gather_texts."""
import json
import os

import numpy as np
import pytest

import wire_model
from conftest import GOLDEN
from plenum_amd.base58 import b58decode_py
from plenum_amd.serialization import serialize_msg_for_signing


@pytest.fixture(scope="module")
def scanned(hostcheck):
    """The corpus, the model's answers and the twin's, computed once."""
    texts = wire_model.corpus()
    model = [wire_model.scan(t) for t in texts]
    buf, off = wire_model.pack_texts(texts, base=3)
    return texts, model, off, wire_model.twin_scan(hostcheck, buf, off)


def _sig_is_64(sig_text):
    return len(b58decode_py(sig_text)) == 64


def test_model_is_sound(scanned):
    texts, model, _, _ = scanned
    accepted = 0
    for t, m in zip(texts, model):
        if m is None:
            continue
        accepted += 1
        ser, idr, sig = m
        d = json.loads(t)
        assert isinstance(d, dict), t
        assert serialize_msg_for_signing(d, ["signature"]) == ser, t
        assert d["identifier"] == idr and d["signature"] == sig, t
        assert len(ser) <= len(t), t
    assert accepted >= 1000


def test_twin_equals_model(scanned):
    texts, model, off, (status, span, sig64, msgs, mlen) = scanned
    n_ok = n_host = 0
    for i, (t, m) in enumerate(zip(texts, model)):
        want_ok = m is not None and _sig_is_64(m[2])
        assert status[i] == (0 if want_ok else 1), (i, t)
        if not want_ok:
            n_host += 1
            assert tuple(span[i]) == (0, 0) and mlen[i] == 0
            continue
        n_ok += 1
        ser, idr, sig = m
        a = int(off[i] - off[0])
        assert msgs[a:a + int(mlen[i])].tobytes() == ser, (i, t)
        s, ln = int(span[i, 0]), int(span[i, 1])
        assert t[s:s + ln] == idr.encode() and t[s - 1:s] == b'"', (i, t)
        assert sig64[i].tobytes() == b58decode_py(sig), (i, t)
    assert n_ok >= 1000 and n_host >= 1000, (n_ok, n_host)


def test_edge_texts_land_where_the_grammar_says(hostcheck):
    """The limits, pinned by hand: the text just inside each is scanned, the one just outside
    goes to the host."""
    edges = wire_model.edge_texts()
    buf, off = wire_model.pack_texts(edges)
    status = wire_model.twin_scan(hostcheck, buf, off)[0]
    want = [0, 0, 1,  # 4095, 4096, 4097 bytes
            0, 1,     # 32, 33 members
            0, 1, 0, 1,  # depth 8, 9 (arrays, then objects)
            0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]  # numbers
    assert status[:len(want)].tolist() == want
    by_text = dict(zip(edges, status.tolist()))
    assert by_text[b"{}"] == 1 and by_text[b""] == 1 and by_text[b"7"] == 1
    assert sum(by_text[t] == 0 for t in edges if b"\\u0041" in t) == 0
    assert all(by_text[t] == (wire_model.scan(t) is None or not _sig_is_64(wire_model.scan(t)[2])) for t in edges)


def test_reference_serializer_kats(hostcheck):
    kats = json.load(open(os.path.join(GOLDEN, "serializer_kat.json")))
    cases = kats["cases"] if isinstance(kats, dict) else kats
    sig = wire_model._rand_sig(__import__("random").Random(1))
    used = 0
    for c in cases:
        if "bytes_hex" not in c or not isinstance(c.get("msg"), dict) or c.get("ignore") != ["signature"]:
            continue
        d = dict(c["msg"], signature=sig)
        had_idr = "identifier" in d
        d.setdefault("identifier", "kat")
        text = json.dumps(d).encode()
        m = wire_model.scan(text)
        if m is None:
            continue
        buf, off = wire_model.pack_texts([text])
        status, _, _, msgs, mlen = wire_model.twin_scan(hostcheck, buf, off)
        assert status[0] == 0
        got = msgs[:int(mlen[0])].tobytes()
        assert got == m[0] == serialize_msg_for_signing(d, ["signature"])
        want = bytes.fromhex(c["bytes_hex"])
        if not had_idr:  # the field this test added, taken out again with one of its separators
            s, f = got.decode(), "identifier:kat"
            if s == f:
                s = ""
            elif s.startswith(f + "|"):
                s = s[len(f) + 1:]
            elif s.endswith("|" + f):
                s = s[:-len(f) - 1]
            else:
                assert s.count("|" + f + "|") == 1, c
                s = s.replace("|" + f + "|", "|")
            got = s.encode()
        assert got == want, c
        used += 1
    assert used >= 10


@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("threads", [1, 3, 7])
def test_gather_texts(n, threads):
    from plenum_amd import _hostpack
    texts = wire_model.corpus()[:n]
    total = sum(len(t) for t in texts)
    out = bytearray(total + 64)
    off_b = _hostpack.gather_texts(texts, out, threads)
    off = np.frombuffer(off_b, np.uint64)
    assert len(off) == n + 1 and off[0] == 0
    assert off[1:].tolist() == np.cumsum([len(t) for t in texts]).tolist()
    assert bytes(out[:total]) == b"".join(texts)


def test_gather_texts_refuses_other_types_and_short_buffers():
    from plenum_amd import _hostpack
    assert _hostpack.gather_texts([b"a", "b"], bytearray(16), 2) is None
    assert _hostpack.gather_texts([b"a", bytearray(b"b")], bytearray(16), 2) is None
    assert _hostpack.gather_texts((b"a",), bytearray(16), 2) is None
    assert _hostpack.gather_texts([b"abcd", b"efgh"], bytearray(7), 2) is None
