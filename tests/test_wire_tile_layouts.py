"""The layouts of tests/wire_tile_model.py on the CPU: the model's constants are the source's,
every layout meets the condition it was built for under the model of the kernels' tile walk
(exactly: slack 0 in the first tile, one byte over in the second, 16 tiles, ...), the chunk rules
give the chunks the GPU tests count on, and on every layout the CPU twins (hc_wire_scan,
hc_wire_unwrap) equal the Python models -- tests/test_gpu_wire_tiles.py then holds the kernels
to the twins."""
import os
import random
import re

import numpy as np
import pytest

import node_split_cases as nsc
import wire_model
import wire_tile_model as wtm
import wire_unwrap_model as wum
from conftest import PKG
from plenum_amd.base58 import b58decode_py


# ------------------------------------------------------------------ the constants
def _constant(source, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, source)
    assert m is not None, name
    expr = re.sub(r"(?<=\d)(?:ull|ul|u)\b", "", m.group(1).strip())
    assert re.fullmatch(r"[0-9\s*+\-<()]+", expr), (name, expr)
    return eval(expr, {"__builtins__": {}})  # (digits and operators only)


def test_the_models_constants_are_the_sources():
    hip = open(os.path.join(PKG, "csrc", "edverify.hip")).read()
    scan_h = open(os.path.join(PKG, "csrc", "wire_scan.h")).read()
    assert _constant(hip, "kWireTile") == wtm.TILE == 20416
    assert _constant(hip, "kWireThreads") == wtm.THREADS == 64
    assert _constant(hip, "kWirePad") == wtm.PAD == 16
    assert _constant(scan_h, "kWireMaxText") == wtm.MAX_TEXT == wire_model.MAX_TEXT == 4096
    assert _constant(hip, "kWireChunk") == wtm.CHUNK == 1 << 17
    assert _constant(hip, "kEntChunkBytes") == wtm.ENT_CHUNK_BYTES == 32 << 20
    # both copies of the loop take an item by the same test and step to the next tile alike
    assert hip.count("if (!done && b <= t0 + kWireTile) {") == 2
    assert hip.count("t0 = next & ~15ull;") == 2
    assert hip.count("uint64_t t0 = (off[i0] - base + kWirePad) & ~15ull;") == 2


# ------------------------------------------------------------------ the walk itself
def test_tile_walk_by_hand():
    # three items of 4,096 at a = 16: t0 = 16, all three end inside 16 + TILE
    assert wtm.tile_walk([0, 4096, 8192, 12288], 0, 3) == [(0, 16, 16, 4112), (0, 16, 4112, 8208),
                                                           (0, 16, 8208, 12304)]
    # base 5: a is taken from off[0]; the fifth item of 4,096 ends at 20,496 > 16 + 20,416
    off = wtm.offsets([4096] * 6, base=5)
    walk = wtm.tile_walk(off, 0, 6)
    assert [w[0] for w in walk] == [0, 0, 0, 0, 1, 1] and walk[4][1:] == (16400, 16400, 20496)
    # an alignment of 7: the next tile starts at the 16 bytes at or below the first item left
    off = wtm.offsets([7, 4096, 4096, 4096, 4096, 4096, 4096])
    walk = wtm.tile_walk(off, 1, 7)
    assert walk[0] == (0, 16, 23, 4119) and walk[4] == (1, 16400, 16407, 20503)
    assert [w[0] for w in walk] == [0, 0, 0, 0, 1, 1] and walk[5][1] == 16400
    # an over-long item is done before the loop; as the first lane it costs an empty first tile
    off = wtm.offsets([wtm.HUGE, 300, 300])
    assert wtm.tile_walk(off, 0, 3) == [(-1, None, 16, 16 + wtm.HUGE), (1, 16 + wtm.HUGE, 16 + wtm.HUGE, 316 + wtm.HUGE),
                                        (1, 16 + wtm.HUGE, 316 + wtm.HUGE, 616 + wtm.HUGE)]
    assert wtm.tiles_per_workgroup(off, 0, 3) == [2] and wtm.tiles_per_workgroup(wtm.offsets([wtm.OVER]), 0, 1) == [1]
    # a launch from `first`: the workgroups are counted from there
    off = wtm.offsets([300] * 130)
    assert len(wtm.tile_walk(off, 64, 130)) == 66 and wtm.tiles_per_workgroup(off, 1, 130) == [1, 1, 1]


def test_item_chunks():
    c = wtm.CHUNK
    assert wtm.item_chunks(0) == []
    assert wtm.item_chunks(c) == [(0, c)]
    assert wtm.item_chunks(c + 1) == [(0, c), (c, c + 1)]
    assert wtm.item_chunks(2 * c + 3) == [(0, c), (c, 2 * c), (2 * c, 2 * c + 3)]


def test_the_item_chunk_cases_cross_their_boundaries():
    c = wtm.CHUNK
    cases = wtm.item_chunk_cases()
    assert [len(wtm.item_chunks(n)) for n, _ in cases.values()] == [1, 2, 2, 3, 2, 2, 2]
    for name, (n, spec) in cases.items():
        assert min(spec) == c - 70 and all(wtm.MIN_LEN <= spec[i] < 1000 for i in range(c - 70, c - 1))
        if name != "second chunk empty":
            assert max(spec) == min(n, (2 * c if n > 2 * c else c) + 70) - 1
    n, spec = cases["second chunk empty"]
    assert n == c + 130 and all(spec[i] == 0 for i in range(c, n))  # no byte of the second chunk to upload
    n, spec = cases["over-long across"]
    assert spec[c - 1] > wtm.MAX_TEXT < spec[c] and spec[c - 2] <= wtm.MAX_TEXT >= spec[c + 1]
    n, spec = cases["4096 across"]
    assert spec[c - 1] == spec[c] == wtm.MAX_TEXT


def test_entry_chunks():
    b = wtm.ENT_CHUNK_BYTES
    assert wtm.entry_chunks([7]) == []
    assert wtm.entry_chunks([0, 10, 20]) == [(0, 2)]
    assert wtm.entry_chunks([3, b + 3, b + 4]) == [(0, 1), (1, 2)]           # an entry ending on the bound belongs
    assert wtm.entry_chunks([3, b + 4, b + 5]) == [(0, 1), (1, 2)]           # one over it: a chunk of its own
    assert wtm.entry_chunks([0, 5, b + 1, b + 2]) == [(0, 1), (1, 3)]
    assert wtm.entry_chunks([0, 0, 0, 0]) == [(0, 3)]                        # a chunk with no bytes
    assert wtm.entry_chunks([0, b, b, 2 * b, 2 * b + 1]) == [(0, 2), (2, 3), (3, 4)]


def test_the_entry_chunk_layout_has_its_four_chunks():
    """The 64 MiB layout of the GPU test, by lengths alone."""
    entries = wtm.entry_chunk_layout(nsc.count_entries())
    assert len(entries) == 74
    for base in (0, 3):
        off = wtm.offsets([len(e) for e in entries], base)
        assert off[25] == off[0] + wtm.ENT_CHUNK_BYTES and off[50] - off[49] == wtm.ENT_CHUNK_BYTES + 5
        assert wtm.entry_chunks(off) == wtm.ENTRY_CHUNKS_WANT == [(0, 25), (25, 49), (49, 50), (50, 74)]
    assert len(wtm.junk_propagate(1000)) == 1000
    assert wum.split(wtm.junk_propagate(1000)) is None and wum.unwrap(wtm.junk_propagate(1000), 0)[0] == wum.NONE


# ------------------------------------------------------------------ texts of an exact length
@pytest.mark.parametrize("total", [wtm.MIN_LEN, 225, 1000, 4095, 4096])
def test_exact_length_texts_are_requests_in_every_form(total):
    t = wtm.request_text(total, "idr3", 17)
    p = wtm.propagate_body(total, "idr3", 17)
    m = wtm.member_body(total, "idr3", 17)
    assert len(t) == len(p) == len(m) == total
    ser, idr, sig = wire_model.scan(t)
    assert idr == "idr3" and len(b58decode_py(sig)) == 64 and len(ser) <= total
    for body, esc in ((t, 0), (p, 0), (m, 1)):
        cls, out = wum.unwrap(body, esc)
        assert cls == wum.REQUEST and len(out) == total
        assert wire_model.scan(out)[1:] == (idr, sig)
    assert wire_model.scan(wtm.request_text(total, "idr3", 18))[0] != ser  # the padding differs per item


def test_over_long_texts_are_requests_but_for_their_length():
    for total in (wtm.OVER, wtm.HUGE):
        t = wtm.request_text(total)
        assert len(t) == total and wire_model.scan(t) is None
        assert wum.unwrap(wtm.propagate_body(total), 0)[0] == wum.HOST
        assert wum.unwrap(wtm.member_body(total), 1)[0] == wum.HOST
    with pytest.raises(ValueError):
        wtm.request_text(100)


# ------------------------------------------------------------------ the layouts' conditions
def _walk(lengths, base=0):
    off = wtm.offsets(lengths, base)
    return off, wtm.tile_walk(off, 0, len(lengths))


@pytest.mark.parametrize("base", [0, 5])
def test_l1_every_alignment_and_slack_is_met(base):
    lengths, cases = wtm.l1_edge_sweep()
    assert len(lengths) % wtm.THREADS == 0 and max(lengths) <= wtm.MAX_TEXT and min(lengths) >= wtm.MIN_LEN
    off, walk = _walk(lengths, base)
    assert sorted((k, al, sl) for _, k, al, sl in cases) == sorted(
        (k, al, sl) for k in (40, 63) for al in (0, 1, 7, 8, 15) for sl in (0, 1, 15, 16, -1, -15, -16, -17))
    for i0, k, align, slack in cases:
        assert i0 % wtm.THREADS == 0
        wg = walk[i0:i0 + wtm.THREADS]
        t0 = wg[0][1]
        assert wg[0][0] == 0 and wg[0][2] & 15 == align and t0 == wg[0][2] - align
        tile, t0_k, a, b = wg[k]
        assert (t0 + wtm.TILE) - b == slack
        assert all(w[0] == 0 and w[1] == t0 for w in wg[:k])
        if slack >= 0:  # the last item of the first tile, `slack` bytes to spare
            assert tile == 0 and t0_k == t0
            assert all(w[0] == 1 for w in wg[k + 1:])
        else:  # over by -slack bytes: first of the second tile, which starts at its 16 bytes
            assert tile == 1 and t0_k == a & ~15 and a >= t0_k
            assert all(w[0] == 1 and w[1] == t0_k for w in wg[k + 1:])
        if k == 63 and slack < 0:
            assert [w[0] for w in wg] == [0] * 63 + [1]  # the last lane alone waits
    # slack 0 and a deferral by one byte exist at every alignment
    for align in (0, 1, 7, 8, 15):
        assert {sl for _, _, al, sl in cases if al == align} >= {0, -1}


def test_l2_takes_16_tiles():
    lengths, firsts = wtm.l2_full_tiles()
    assert lengths[:64] == [4096] * 64 and sorted(set(lengths[64:])) == [4094, 4095, 4096]
    for base in (0, 5):
        off, walk = _walk(lengths, base)
        assert wtm.tiles_per_workgroup(off, 0, len(lengths)) == [16, 16]
        for i0 in firsts:
            assert [w[0] for w in walk[i0:i0 + 64]] == [k // 4 for k in range(64)]


def test_l3_over_long_items_in_every_lane_position():
    lengths, over = wtm.l3_over_long()
    off, walk = _walk(lengths)
    assert [(i // 64, i % 64, lengths[i]) for i in over] == [
        (1, 0, wtm.OVER), (1, 31, wtm.HUGE), (1, 63, wtm.OVER),
        (2, 0, wtm.HUGE), (2, 31, wtm.OVER), (2, 32, wtm.HUGE), (2, 63, wtm.HUGE),
        (3, 0, wtm.OVER), (3, 1, wtm.OVER)]
    assert all(walk[i][0] == -1 for i in over)
    assert all(walk[i][0] >= 0 and lengths[i] <= wtm.MAX_TEXT for i in range(len(lengths)) if i not in over)
    # a 100 KiB item parts its neighbours into different tiles; as the first lane it leaves tile 0 empty
    assert walk[64 + 30][0] == 0 and walk[64 + 32][0] == 1
    assert [w[0] for w in walk[128:192]] == [-1] + [1] * 30 + [-1, -1] + [2] * 30 + [-1]
    assert walk[128 + 1][1] == walk[128 + 1][2] & ~15
    assert wtm.tiles_per_workgroup(off, 0, len(lengths)) == [1, 2, 3, 2, 1]
    # scannable neighbours on both sides of every run of over-long items
    runs = []
    for i in over:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    assert [b - a for a, b in runs] == [1, 1, 2, 2, 3]  # 127 | 128 and 191 | 192, 193 cross a workgroup boundary
    for a, b in runs:
        assert wtm.MIN_LEN <= lengths[a - 1] <= wtm.MAX_TEXT and wtm.MIN_LEN <= lengths[b] <= wtm.MAX_TEXT


def test_l4_empty_items_where_the_walk_could_trip():
    lengths, marks = wtm.l4_empty_items()
    off, walk = _walk(lengths)
    i = marks["all_empty"]
    assert i % 64 == 0 and lengths[i:i + 64] == [0] * 64 and all(w[0] == 0 and w[2] == w[3] for w in walk[i:i + 64])
    i = marks["ends_tile"]
    tile, t0, a, b = walk[i]
    assert lengths[i] == lengths[i + 1] == 0 and (tile, a, b) == (0, t0 + wtm.TILE, t0 + wtm.TILE)
    assert walk[i + 1][:2] == (0, t0) and walk[i - 1][3] == t0 + wtm.TILE and walk[i + 2][0] == 1
    i = marks["starts_tile"]
    tile, t0, a, b = walk[i]
    assert lengths[i] == 0 and walk[i - 1][0] == -1 and walk[i - 2][0] == 0 and tile == 1 and t0 == a & ~15
    assert walk[i + 1][:2] == (1, t0)
    i = marks["first_lane"]
    assert i % 64 == 0 and lengths[i] == 0 and walk[i][0] == 0
    assert marks["last_of_batch"] == len(lengths) - 1 and lengths[-1] == 0 and len(lengths) % 64 == 0


def test_l5_a_single_item_ends_the_batch_short_of_16_bytes():
    for short in (0, 1, 15):
        lengths = wtm.l5_last_workgroup(short)
        off, walk = _walk(lengths, base=5)
        assert len(lengths) == 65 and wtm.tiles_per_workgroup(off, 0, 65) == [1, 1]
        end = walk[-1][3]
        assert end == wtm.PAD + sum(lengths) and (end + short) % 16 == 0 and (short == 0 or (end + short - 1) % 16)
    assert wtm.all_families()[-65:] == wtm.l5_last_workgroup(15)


def test_the_plain_scan_tests_never_reach_a_second_tile():
    """What tests/test_gpu_wire.py's corpus batches do under the model: 253 bytes a text on
    average, so the 64 items of every workgroup end inside its first tile."""
    corpus = wire_model.corpus()
    for seed, n in ((100 + 4096, 4096), (5, 777), (100 + 65, 65)):
        chosen = random.Random(seed).choices(corpus, k=n)
        off = wtm.offsets([len(t) for t in chosen])
        assert wtm.max_tiles(off) == 1, (seed, n)
        walk = wtm.tile_walk(off, 0, n)
        assert min(w[1] + wtm.TILE - w[3] for w in walk if w[0] == 0) > 1000


# ------------------------------------------------------------------ twin == model on every layout
def _batches():
    out = [(name, k, lengths) for name, group in wtm.families().items() for k, lengths in enumerate(group)]
    return out


def _model_scan_equals_twin(hostcheck, texts, base):
    buf, off = wire_model.pack_texts(texts, base=base)
    status, span, sig64, msgs, mlen = wire_model.twin_scan(hostcheck, buf, off)
    n_ok = 0
    for i, t in enumerate(texts):
        m = wire_model.scan(t)
        ok = m is not None and len(b58decode_py(m[2])) == 64
        assert status[i] == (0 if ok else 1), (i, len(t))
        if not ok:
            assert tuple(span[i]) == (0, 0) and mlen[i] == 0
            continue
        n_ok += 1
        ser, idr, sig = m
        a = int(off[i] - off[0])
        assert msgs[a:a + int(mlen[i])].tobytes() == ser, i
        s, ln = int(span[i, 0]), int(span[i, 1])
        assert t[s:s + ln] == idr.encode() and sig64[i].tobytes() == b58decode_py(sig), i
    return n_ok


@pytest.mark.parametrize("name,k,lengths", _batches(), ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_twin_equals_model_on_the_layout(hostcheck, name, k, lengths):
    texts = wtm.texts(lengths)
    assert [len(t) for t in texts] == lengths
    n_ok = _model_scan_equals_twin(hostcheck, texts, base=5)
    # every item of a scannable length is scanned with status 0: the layouts test tiles, not refusals
    assert n_ok == sum(0 < n <= wtm.MAX_TEXT for n in lengths)


@pytest.mark.parametrize("name,k,lengths", _batches(), ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_twins_equal_models_on_the_node_form(hostcheck, name, k, lengths):
    msgs = wtm.node_messages(lengths)
    assert [len(b) for b, _ in msgs] == lengths
    buf, off = wire_model.pack_texts([b for b, _ in msgs], base=3)
    esc = np.array([e for _, e in msgs], np.uint8)
    cls, out = wum.twin_unwrap(hostcheck, buf[3:], off - off[0], esc)
    want = [wum.unwrap(b, e) for b, e in msgs]
    assert cls.tolist() == [c for c, _ in want]
    assert out.tobytes() == b"".join(o for _, o in want)
    assert [c for c, _ in want] == [wum.REQUEST if 0 < n <= wtm.MAX_TEXT else wum.HOST for n in lengths]
    if any(e for _, e in msgs):
        assert {e for (b, e) in msgs if 0 < len(b) <= wtm.MAX_TEXT} == {0, 1}
    n_ok = _model_scan_equals_twin(hostcheck, [o for _, o in want], base=0)
    assert n_ok == sum(0 < n <= wtm.MAX_TEXT for n in lengths)
