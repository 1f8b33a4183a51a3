"""The GPU-only parts of the wire path restated in Python, and the layouts that drive them to
their edges: the LDS tile walk that edv_wire_scan_kernel and edv_wire_unwrap_kernel share
(csrc/edverify.hip; each holds its own copy of the loop) and the host's chunked launches
(kWireChunk items per scan launch, kEntChunkBytes of entries per count launch).  The parsing is
held to the CPU twins elsewhere; the twins have no tiles and no chunks, so a layout here is
chosen by what the walk does with it, and tests/test_wire_tile_layouts.py asserts that it does.

A layout is a list of item lengths (0: an empty item) with marks for the tests; texts() makes
them bare requests, node_messages() a mix of bare requests, PROPAGATEs (esc 0) and escaped BATCH
member bodies (esc 1) of exactly those lengths."""
import bisect
import random

import wire_model
import wire_unwrap_model as wum

TILE = 20 * 1024 - 64    # kWireTile
THREADS = 64             # kWireThreads: items per workgroup
PAD = 16                 # kWirePad
MAX_TEXT = 4096          # kWireMaxText
CHUNK = 1 << 17          # kWireChunk
ENT_CHUNK_BYTES = 32 << 20  # kEntChunkBytes

MIN_LEN = 224            # every form of a request fits (the escaped PROPAGATE is the longest)
OVER = MAX_TEXT + 1
HUGE = 100 * 1024


# ------------------------------------------------------------------ the walk and the chunks
def tile_walk(off, first, end):
    """One launch over the items [first, end) of a batch with offsets off[n + 1]: per item
    (tile, t0, a, b) -- the iteration of its workgroup's loop that parses it (-1 for an item
    over MAX_TEXT, marked for the host before the loop) and that tile's start; a, b are the
    item's bounds in the padded device buffer.  (-1, None, a, b) for an over-long item."""
    base = int(off[0])
    out = []
    for i0 in range(first, end, THREADS):
        i1 = min(i0 + THREADS, end)
        ab = [(int(off[i]) - base + PAD, int(off[i + 1]) - base + PAD) for i in range(i0, i1)]
        res = [None] * len(ab)
        todo = []
        for k, (a, b) in enumerate(ab):
            if b - a > MAX_TEXT:
                res[k] = (-1, None, a, b)
            else:
                todo.append(k)
        t0 = ab[0][0] & ~15
        tile = 0
        while True:
            rest = []
            for k in todo:
                a, b = ab[k]
                if b <= t0 + TILE:
                    res[k] = (tile, t0, a, b)
                else:
                    rest.append(k)
            if not rest:
                break
            assert len(rest) < len(todo) or tile == 0, "a tile after the first finishes at least one item"
            todo = rest
            t0 = min(ab[k][0] for k in todo) & ~15
            tile += 1
        out += res
    return out


def tiles_per_workgroup(off, first, end):
    """Loop iterations of every workgroup of the launch (1 where nothing is parsed)."""
    walk = tile_walk(off, first, end)
    return [max(1, 1 + max(w[0] for w in walk[k:k + THREADS])) for k in range(0, len(walk), THREADS)]


def max_tiles(off, first=0, end=None):
    end = len(off) - 1 if end is None else end
    return max(tiles_per_workgroup(off, first, end), default=0)


def offsets(lengths, base=0):
    off = [base]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def item_chunks(n):
    """[(first, end)] of the scan launches over n items."""
    return [(c0, min(c0 + CHUNK, n)) for c0 in range(0, n, CHUNK)]


def entry_chunks(entry_off):
    """[(e0, e1)] of the count launches (edv_wire_scan_entries): the entries from e0 that end
    at or before entry_off[e0] + ENT_CHUNK_BYTES; one entry over the bound is a chunk of its own."""
    entry_off = [int(x) for x in entry_off]
    n_e = len(entry_off) - 1
    out, e0 = [], 0
    while e0 < n_e:
        e1 = bisect.bisect_right(entry_off, entry_off[e0] + ENT_CHUNK_BYTES, e0 + 1, n_e + 1) - 1
        if e1 <= e0:
            e1 = e0 + 1
        out.append((e0, e1))
        e0 = e1
    return out


# ------------------------------------------------------------------ texts of an exact length
_PAD_CHARS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ,:|[]{}"


def _padding(k, seed):
    """k bytes that differ from item to item (a serialization read from another item's place in
    the tile shows)."""
    s = seed % len(_PAD_CHARS)
    rot = _PAD_CHARS[s:] + _PAD_CHARS[:s]
    return (rot * (k // len(rot) + 1))[:k]


def _sig(seed):
    return wire_model._rand_sig(random.Random(1000 + seed))


def request_dict(idr, seed, pad):
    return {"identifier": idr, "signature": _sig(seed), "p": _padding(pad, seed)}


def request_text(total, idr="idr", seed=0):
    """A request the scanner accepts, exactly `total` bytes, padded through a string member
    (as wire_model.edge_texts's padded())."""
    head = '{"identifier":"%s","signature":"%s","p":"' % (idr, _sig(seed))
    k = total - len(head) - 2
    if k < 0:
        raise ValueError("a request of %d bytes is too short" % total)
    return (head + _padding(k, seed) + '"}').encode()


def propagate_body(total, idr="idr", seed=0):
    """The same request inside a PROPAGATE (nodeloop.propagate_text), exactly `total` bytes: esc 0."""
    from plenum_amd.nodeloop import propagate_text
    short = len(propagate_text(request_dict(idr, seed, 0), "c%d" % (seed % 10)))
    if total < short:
        raise ValueError("a PROPAGATE of %d bytes is too short" % total)
    out = propagate_text(request_dict(idr, seed, total - short), "c%d" % (seed % 10)).encode()
    assert len(out) == total
    return out


def member_body(total, idr="idr", seed=0):
    """That PROPAGATE as the still escaped body of a BATCH member string (nodeloop.batch_text,
    cut out as the splitter does), exactly `total` bytes: esc 1."""
    from plenum_amd.nodeloop import batch_text, propagate_text

    def body(pad):
        (b,) = wum.split(batch_text([propagate_text(request_dict(idr, seed, pad), "c%d" % (seed % 10))]).encode())
        return b

    short = len(body(0))
    if total < short:
        raise ValueError("a member body of %d bytes is too short" % total)
    out = body(total - short)
    assert len(out) == total
    return out


def item(i, n):
    """Item i of a layout as a bare request text of n bytes (an over-long one is a request but
    for its length; 0: the empty item)."""
    return b"" if n == 0 else request_text(n, "idr%d" % (i % 7), i)


def node_item(i, n):
    """Item i of a layout as a node message (body of n bytes, esc): a bare request, a PROPAGATE
    or an escaped member, by i."""
    idr = "idr%d" % (i % 7)
    if n == 0:
        return b"", i % 2
    if i % 3 == 0:
        return request_text(n, idr, i), 0
    if i % 3 == 1:
        return propagate_body(n, idr, i), 0
    return member_body(n, idr, i), 1


def texts(lengths):
    return [item(i, n) for i, n in enumerate(lengths)]


def node_messages(lengths):
    return [node_item(i, n) for i, n in enumerate(lengths)]


# ------------------------------------------------------------------ the layouts
def _spread(total, count, lo=MIN_LEN, hi=MAX_TEXT):
    """`count` lengths in [lo, hi] that sum to `total`, uneven."""
    assert count * lo <= total <= count * hi, (total, count)
    out = [lo] * count
    left = total - count * lo
    k = 0
    while left:
        add = min(left, hi - out[k % count], 97 + 131 * (k % 5))
        out[k % count] += add
        left -= add
        k += 1
    return out


L1_ALIGNS = (0, 1, 7, 8, 15)
L1_SLACKS = (0, 1, 15, 16, -1, -15, -16, -17)
L1_LANES = (40, 63)


def l1_edge_sweep():
    """(lengths, cases): per alignment, slack and lane k two workgroups -- one whose bytes set the
    alignment a & 15 of the next one's first item, and one whose item k ends `slack` bytes before
    the first tile's end (negative: after it, so the item waits for the second tile).
    cases: (first item of the second workgroup, k, alignment, slack)."""
    lengths, cases = [], []
    for k in L1_LANES:
        for align in L1_ALIGNS:
            for slack in L1_SLACKS:
                have = sum(lengths) & 15
                fill = [MIN_LEN + (j % 5) for j in range(THREADS - 1)]
                fill.append(MIN_LEN + 16 + (align - have - sum(fill) - MIN_LEN) % 16)
                lengths += fill
                assert sum(lengths) & 15 == align
                cases.append((len(lengths), k, align, slack))
                # the items 0 .. k end at t0 + TILE - slack, and t0 = a - align
                lengths += _spread(TILE - slack - align, k + 1)
                lengths += [MIN_LEN + 3 * j for j in range(THREADS - 1 - k)]
    return lengths, cases


def l2_full_tiles():
    """(lengths, first items): 64 items of 4,096 bytes, then 64 of 4,096 - (k % 3): four to a
    tile, 16 tiles each."""
    return [MAX_TEXT] * THREADS + [MAX_TEXT - (k % 3) for k in range(THREADS)], [0, THREADS]


def l3_over_long():
    """(lengths, over-long items): items of 4,097 and 100 KiB bytes as the first, a middle and
    the last lane of a workgroup, two of them adjacent inside a workgroup and two across a
    workgroup boundary, scannable neighbours on both sides."""
    def wg(special):
        return [special.get(k, MIN_LEN + 7 * (k % 9)) for k in range(THREADS)]

    lengths = wg({})
    lengths += wg({0: OVER, 31: HUGE, 63: OVER})
    lengths += wg({0: HUGE, 31: OVER, 32: HUGE, 63: HUGE})
    lengths += wg({0: OVER, 1: OVER})
    lengths += wg({})
    return lengths, [i for i, n in enumerate(lengths) if n > MAX_TEXT]


def l4_empty_items():
    """(lengths, marks): a workgroup of 64 empty items; an empty item that ends a tile (it lies
    at t0 + TILE exactly) with a second one behind it; an empty item that starts the next tile
    (behind an over-long one, the only place an empty item can wait); an empty first lane; and
    an empty last item of the batch.  marks: name -> item."""
    lengths = [MIN_LEN + k for k in range(THREADS)]
    marks = {"all_empty": len(lengths)}
    lengths += [0] * THREADS
    align = sum(lengths) & 15
    first = len(lengths)
    marks["ends_tile"] = first + 40
    lengths += _spread(TILE - align, 40) + [0, 0] + [MIN_LEN] * (THREADS - 42)
    marks["starts_tile"] = len(lengths) + 21
    lengths += [MIN_LEN + k for k in range(20)] + [HUGE, 0] + [MIN_LEN + k for k in range(THREADS - 22)]
    marks["first_lane"] = len(lengths)
    lengths += [0] + [MIN_LEN + 2 * k for k in range(THREADS - 2)] + [0]
    marks["last_of_batch"] = len(lengths) - 1
    return lengths, marks


L5_SHORT = (0, 1, 15)


def l5_last_workgroup(short):
    """A full workgroup and a last one of a single item whose end in the device buffer is `short`
    bytes before a 16-byte boundary: the tile's last load and the zeroed tail behind the batch."""
    lengths = [MIN_LEN + (k % 4) for k in range(THREADS)]
    lengths.append(MIN_LEN + 16 + (-short - sum(lengths) - MIN_LEN) % 16)
    assert (PAD + sum(lengths) + short) % 16 == 0
    return lengths


def families():
    """name -> [lengths, ...]: one batch per list (L5 is three batches)."""
    return {"L1": [l1_edge_sweep()[0]], "L2": [l2_full_tiles()[0]], "L3": [l3_over_long()[0]],
            "L4": [l4_empty_items()[0]], "L5": [l5_last_workgroup(s) for s in L5_SHORT]}


def all_families():
    """Every family in one batch (L5 once, last: its single-item workgroup ends the batch)."""
    f = families()
    return f["L1"][0] + f["L2"][0] + f["L3"][0] + f["L4"][0] + f["L5"][2]


# ------------------------------------------------------------------ the chunk layouts
def junk_propagate(total):
    """A PROPAGATE without a request, exactly `total` bytes: an entry the splitter leaves whole."""
    head, tail = b'{"op":"PROPAGATE","k":"', b'"}'
    return head + b"z" * (total - len(head) - len(tail)) + tail


def entry_chunk_layout(small):
    """The entries of the 32 MiB test: 24 small ones, a junk PROPAGATE whose end is exactly
    entry_off[0] + ENT_CHUNK_BYTES, 24 small, one entry of ENT_CHUNK_BYTES + 5, 24 small.
    small: the entries to draw the small ones from, in turn (again from the first when they run out)."""
    turn = (list(small) * (72 // len(small) + 1))[:72]
    a, b, c = turn[:24], turn[24:48], turn[48:]
    big = junk_propagate(ENT_CHUNK_BYTES - sum(map(len, a)))
    return a + [big] + b + [junk_propagate(ENT_CHUNK_BYTES + 5)] + c


ENTRY_CHUNKS_WANT = [(0, 25), (25, 49), (49, 50), (50, 74)]


def item_chunk_cases():
    """name -> (n, {item: length}): the batches of the item-chunk tests.  Every item is "{}" (the
    host's) but for those named: requests in the 70 items on either side of each chunk boundary,
    and what the name says."""
    def around(n, *boundaries):
        return {i: MIN_LEN + 13 * (i % 50) for b in boundaries for i in range(b - 70, min(n, b + 70))}

    c = CHUNK
    return {
        "n=2^17": (c, around(c, c)),
        "n=2^17+1": (c + 1, around(c + 1, c)),
        "n=2^17+65": (c + 65, around(c + 65, c)),
        "n=2*2^17+3": (2 * c + 3, around(2 * c + 3, c, 2 * c)),
        "second chunk empty": (c + 130, {**around(c, c), **{i: 0 for i in range(c, c + 130)}}),
        "over-long across": (c + 65, {**around(c + 65, c), c - 1: HUGE, c: OVER}),
        "4096 across": (c + 65, {**around(c + 65, c), c - 1: MAX_TEXT, c: MAX_TEXT}),
    }
