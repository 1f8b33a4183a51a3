"""The GPU-only parts of the wire path on the MI355X: the LDS tile walk of edv_wire_scan_kernel
and edv_wire_unwrap_kernel at its edges (tests/wire_tile_model.py's layouts: an item ending on a
tile's last byte, one byte over, 16 tiles to a workgroup, over-long and empty items in every
position), and the host's chunked launches (2^17 items per scan launch, 32 MiB of entries per
count launch) across their boundaries.  Everything is held to the CPU twins byte for byte, whole
buffers at a time; tests/test_wire_tile_layouts.py holds the twins to the Python models on the
same layouts and asserts what each layout does to the walk."""
import functools

import numpy as np
import pytest

import node_split_cases as nsc
import wire_model
import wire_tile_model as wtm
import wire_unwrap_model as wum
from plenum_amd import _hostpack
from test_gpu_wire import _own_keys, nym_batch, nym_expect  # noqa: F401  (the fixtures are used by name)
from wire_idents_double import ident_strings

pytestmark = pytest.mark.gpu

C = wtm.CHUNK
NO_ID = 0xFFFFFFFF
FILL = b"{}"  # an item the scan leaves to the host


# ------------------------------------------------------------------ whole-buffer comparison
def _message_bytes(start, mlen, items):
    """The positions of every message byte of `items` (message i at start[i], mlen[i] long)."""
    lens = mlen[items].astype(np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(lens) - lens
    return np.repeat(start[items].astype(np.int64) - first, lens) + np.arange(total, dtype=np.int64)


def _same_scan(got, want, start):
    """(status, span, sig64, msgs, mlen) of the device against the reference: every status, span
    and length, and the signature and every message byte of the status-0 items."""
    status, span, sig, msgs, mlen = got
    w_status, w_span, w_sig, w_msgs, w_mlen = want
    assert np.array_equal(status, w_status), np.flatnonzero(status != w_status)[:8]
    assert np.array_equal(span, w_span), np.flatnonzero((span != w_span).any(axis=1))[:8]
    assert np.array_equal(mlen, w_mlen), np.flatnonzero(mlen != w_mlen)[:8]
    ok = np.flatnonzero(status == 0)
    assert np.array_equal(sig[ok], w_sig[ok]), ok[(sig[ok] != w_sig[ok]).any(axis=1)][:8]
    at = _message_bytes(start, mlen, ok)
    differ = msgs[at] != w_msgs[at]
    assert not differ.any(), (int(differ.sum()), at[differ][:8])
    return ok


def _check_scan(eng, hostcheck, texts, base):
    buf, off = wire_model.pack_texts(texts, base=base)
    status, span = eng.wire_scan(buf, off)
    sig, msgs, mlen = eng.wire_readback()
    _same_scan((status, span, sig, msgs, mlen), wire_model.twin_scan(hostcheck, buf, off), off[:-1] - off[0])
    return status


def _check_node(eng, hostcheck, msgs_in, base):
    buf, off = wire_model.pack_texts([b for b, _ in msgs_in], base=base)
    esc = np.array([e for _, e in msgs_in], np.uint8)
    cls, status, span = eng.wire_scan_node(buf, off, esc)
    sig, out, mlen = eng.wire_readback()
    t_cls, t_text = wum.twin_unwrap(hostcheck, buf[base:], off - off[0], esc)
    assert np.array_equal(cls, t_cls), np.flatnonzero(cls != t_cls)[:8]
    _same_scan((status, span, sig, out, mlen), wire_model.twin_scan(hostcheck, t_text, off - off[0]),
               off[:-1] - off[0])
    assert not (status[cls != 0] == 0).any()  # only a request is ever scanned
    return cls, status


# ------------------------------------------------------------------ tiles
@functools.lru_cache(maxsize=None)
def _family(name, node):
    return [(wtm.node_messages(ls) if node else wtm.texts(ls), ls) for ls in wtm.families()[name]]


@functools.lru_cache(maxsize=None)
def _everything(node):
    ls = wtm.all_families()
    return (wtm.node_messages(ls) if node else wtm.texts(ls)), ls


def _scannable(lengths):
    return sum(0 < n <= wtm.MAX_TEXT for n in lengths)


@pytest.mark.parametrize("base", [0, 5])
@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4", "L5"])
def test_tile_layouts_through_the_scan(gpu_engine, hostcheck, name, base):
    for texts, lengths in _family(name, False):
        status = _check_scan(gpu_engine, hostcheck, texts, base)
        assert int((status == 0).sum()) == _scannable(lengths)


@pytest.mark.parametrize("base", [0, 5])
def test_every_tile_layout_in_one_scan(gpu_engine, hostcheck, base):
    texts, lengths = _everything(False)
    status = _check_scan(gpu_engine, hostcheck, texts, base)
    assert int((status == 0).sum()) == _scannable(lengths)


@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4", "L5"])
def test_tile_layouts_through_the_unwrap_and_the_scan(gpu_engine, hostcheck, name):
    for msgs, lengths in _family(name, True):
        cls, status = _check_node(gpu_engine, hostcheck, msgs, 3)
        assert int((status == 0).sum()) == int((cls == 0).sum()) == _scannable(lengths)


def test_every_tile_layout_in_one_node_scan(gpu_engine, hostcheck):
    msgs, lengths = _everything(True)
    cls, status = _check_node(gpu_engine, hostcheck, msgs, 0)
    assert int((status == 0).sum()) == int((cls == 0).sum()) == _scannable(lengths)


# ------------------------------------------------------------------ item chunks
_CHUNK_CASES = wtm.item_chunk_cases()


@pytest.mark.parametrize("case", list(_CHUNK_CASES))
def test_item_chunks_through_the_scan(gpu_engine, hostcheck, case):
    n, spec = _CHUNK_CASES[case]
    texts = [FILL] * n
    for i, length in spec.items():
        texts[i] = wtm.item(i, length)
    status = _check_scan(gpu_engine, hostcheck, texts, 5 * (n % 2))
    want_ok = sorted(i for i, length in spec.items() if 0 < length <= wtm.MAX_TEXT)
    assert np.flatnonzero(status == 0).tolist() == want_ok
    assert (status[:C] == 0).any() and (n == C or case == "second chunk empty" or (status[C:] == 0).any())


@pytest.mark.parametrize("case", list(_CHUNK_CASES))
def test_item_chunks_through_the_unwrap_and_the_scan(gpu_engine, hostcheck, case):
    n, spec = _CHUNK_CASES[case]
    msgs = [(FILL, 0)] * n
    for i, length in spec.items():
        msgs[i] = wtm.node_item(i, length)
    assert {e for i, (_, e) in enumerate(msgs) if i in spec} == {0, 1}
    cls, status = _check_node(gpu_engine, hostcheck, msgs, 5 * (n % 2))
    want_ok = sorted(i for i, length in spec.items() if 0 < length <= wtm.MAX_TEXT)
    assert np.flatnonzero(status == 0).tolist() == np.flatnonzero(cls == 0).tolist() == want_ok


def _check_entries(eng, entries, base):
    """wire_scan_entries over the entries against the host split and wire_scan_node, as
    test_gpu_wire_split._check, whole buffers at a time."""
    text, eoff = nsc.pack(entries, base)
    cls, status, span, esc, entry, at, off = eng.wire_scan_entries(text, eoff)
    raw = eng.wire_raw_readback()
    sig, msgs, mlen = eng.wire_readback()
    h_off, h_esc, h_entry, h_bodies = nsc.host_split(entries)
    assert np.array_equal(off, h_off) and np.array_equal(esc, h_esc) and np.array_equal(entry, h_entry)
    assert np.array_equal(raw, h_bodies)
    # the bodies lie at `at` in the caller's text: the long ones slice by slice, the rest in one go
    lens = np.diff(off).astype(np.int64)
    for i in np.flatnonzero(lens > 1 << 20).tolist():
        a = int(at[i])
        assert np.array_equal(text[a:a + int(lens[i])], h_bodies[int(off[i]):int(off[i + 1])]), i
    short = np.flatnonzero(lens <= 1 << 20)
    assert np.array_equal(text[_message_bytes(at, lens, short)], h_bodies[_message_bytes(off[:-1], lens, short)])
    n_cls, n_status, n_span = eng.wire_scan_node(h_bodies, h_off, h_esc)
    n_sig, n_msgs, n_mlen = eng.wire_readback()
    assert np.array_equal(cls, n_cls)
    _same_scan((status, span, sig, msgs, mlen), (n_status, n_span, n_sig, n_msgs, n_mlen), off[:-1])
    return cls, status, esc, entry


def test_more_members_than_one_scan_launch_takes(gpu_engine):
    """1,100 BATCHes of 130 members: 143,000 messages, so edv_wire_scan_entries launches the
    unwrap and the scan twice.  The members are tiny but for the three BATCHes around message
    2^17, whose members are PROPAGATEs of requests (scanned on both sides of the boundary)."""
    from plenum_amd.nodeloop import batch_text, propagate_text
    tiny = [b"" if j % 7 == 3 else b'{\\"n\\":%d,\\"s\\":\\"a\\\\\\\\b\\/c\\"}' % j for j in range(130)]
    entries = [nsc.batch_of(tiny[k % 5:] + tiny[:k % 5]) for k in range(1100)]
    for k in (1007, 1008, 1009):
        entries[k] = batch_text([propagate_text(wtm.request_dict("idr%d" % (j % 7), 130 * k + j, 3 * (j % 40)),
                                                "c%d" % j) for j in range(130)]).encode()
    cls, status, esc, entry = _check_entries(gpu_engine, entries, base=3)
    assert len(esc) == 143000 > C and esc.all() and entry[C] == 1008
    assert np.flatnonzero(status == 0).tolist() == list(range(130 * 1007, 130 * 1010))
    assert (status[:C] == 0).any() and (status[C:] == 0).any()


# ------------------------------------------------------------------ verdicts across the boundary
def test_verdicts_and_identifiers_across_the_item_chunk(gpu_engine, nym_batch, nym_expect):  # noqa: F811
    """The 4,096 GPU-signed NYM texts, every third S corrupted, repeated to 2^17 + 128 items --
    every item is live: wire_verify against the C oracle's verdicts tiled, wire_idents against
    the host pass, wire_verify_idents against wire_verify."""
    pk, _, _, _, texts, kidx, _, _ = nym_batch
    n = C + 128
    reps = -(-n // len(texts))
    live = (texts * reps)[:n]
    kidx_n = np.tile(kidx, reps)[:n]
    want = np.tile(nym_expect, reps)[:n]
    buf, off = wire_model.pack_texts(live)
    with _own_keys(gpu_engine):
        first = gpu_engine.keys_add(pk)
        status, span = gpu_engine.wire_scan(buf, off)
        assert not status.any()
        ids = (kidx_n + first).astype(np.uint32)
        mixed = np.where(np.arange(n) % 2 == 0, ids, np.uint32(NO_ID)).astype(np.uint32)
        verdicts = gpu_engine.wire_verify(mixed, pk[kidx_n])
        assert np.array_equal(verdicts, want), np.flatnonzero(verdicts != want)[:8]
        assert want[C:].any() and not want[C:].all()
        uidx, uniq_item = gpu_engine.wire_idents()
        want_b, want_uniq = _hostpack.wire_idents(buf, off.tobytes(), status, span)
        assert np.array_equal(uidx, np.frombuffer(want_b, np.uint32))
        assert ident_strings(buf, off, span, uniq_item) == want_uniq and len(uniq_item) == 8
        kid_u = (kidx_n[uniq_item] + first).astype(np.uint32)
        assert np.array_equal(gpu_engine.wire_verify_idents(kid_u), gpu_engine.wire_verify(ids))
        assert np.array_equal(gpu_engine.wire_verify_idents(kid_u), want)


def test_authenticate_wire_batch_across_the_item_chunk(gpu_engine, nym_batch, nym_expect):  # noqa: F811
    """authenticate_wire_batch over 2^17 + 64 live texts end to end against the oracle's verdicts."""
    from plenum_amd.client_authn import GpuAuthNr
    _, idrs, vks, _, texts, kidx, _, _ = nym_batch
    n = C + 64
    reps = -(-n // len(texts))
    live = (texts * reps)[:n]
    with _own_keys(gpu_engine):
        a = GpuAuthNr(engine=gpu_engine, max_keys=16)
        for idr, vk in zip(idrs, vks):
            a.addIdr(idr, vk)
        a.keys_settle()
        got = a.authenticate_wire_batch(live)
        assert a.stats["wire_host_items"] == 0 and a.stats["wire_items"] == n
    accepted = np.array([isinstance(g, str) for g in got])
    assert np.array_equal(accepted, np.tile(nym_expect, reps)[:n])
    who = np.tile(kidx, reps)[:n]
    assert all(g == idrs[who[i]] for i, g in enumerate(got) if isinstance(g, str))


# ------------------------------------------------------------------ entry chunks
def test_entry_chunks_of_32_mib(gpu_engine):
    """64 MiB of entries in the four count launches [(0, 25), (25, 49), (49, 50), (50, 74)]: a
    chunk that ends on the bound exactly, a chunk that starts at e0 > 0, an entry over the bound
    as a chunk of its own, and the copy of two 32 MiB messages."""
    entries = wtm.entry_chunk_layout(nsc.count_entries())
    assert wtm.entry_chunks(wtm.offsets([len(e) for e in entries], 3)) == wtm.ENTRY_CHUNKS_WANT
    cls, status, esc, entry = _check_entries(gpu_engine, entries, base=3)
    for e in (24, 49):  # the two long entries: one message each, the host's
        (i,) = np.flatnonzero(entry == e).tolist()
        assert esc[i] == 0 and cls[i] == 1 and status[i] == 1
    # BATCHes are split in every chunk
    members = np.bincount(entry[esc == 1], minlength=74)
    assert members[:24].sum() > 50 and members[25:49].sum() > 50 and members[50:].sum() > 50
