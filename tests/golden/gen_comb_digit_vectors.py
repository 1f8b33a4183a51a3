"""Generate Ed25519 vectors whose scalars sit on the comb's digit edges.

The verify kernels compute [h](-A) + [S]B with signed radix-2^W digits
(csrc/comb.h): y = x + bias, digit_i = ((y >> W*i) & (2^W - 1)) - 2^(W-1).  A
random scalar reads a row's last entry (digit -2^(W-1)), its identity (digit
0) or its neighbours with probability 2^-W, which at the shipped base window
W = 24 no test batch reaches.  This script searches for valid signatures
whose S or h has exactly such a digit in a chosen row:

  target = (kind, W, row, v)   kind "S" at W = 24 (the shipped base table) and
                               W = 16 (the host build's); kind "h" at W = 10,
                               14 and 16 (the key tables)
  v in {-2^(W-1), -2^(W-1)+1, -1, 0, 1, 2^(W-1)-1}

over a few fixed keys and fixed nonces r: R and A stay fixed and a counter in
the message moves h = SHA-512(R || A || M) mod L and S = r + h a mod L.  A
target is reachable when a uniform scalar below L has that digit with
probability at least 2^-26 (counted exactly); the others (the top rows reach
only small non-negative digits, some digits need x >= 2^252) are listed in
the labels as unreachable.  For every target the item with the lowest counter
is kept, plus a twin with one bit of S flipped (the low bit of the targeted
row for S targets, bit 0 for h targets), which must be rejected.

Deterministic: counters are scanned in fixed rounds and the lowest counter
wins, whatever the number of worker processes.  Python, hashlib and numpy
only for the search; the expected verdicts are libsodium 1.0.18's own return
values, as in gen_golden.py.

Outputs: comb_digit_edge.npz (sig, pk, msgs, off, expect) and
comb_digit_edge_labels.json.

Run:  python3 tests/golden/gen_comb_digit_vectors.py   (minutes on 16 CPUs; not run by tests)
"""
import functools
import hashlib
import json
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edwards as E  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
L = E.L
S_WINDOWS = (24, 16)
H_WINDOWS = (10, 14, 16)
MIN_LOG2_PROB = -26
CHUNK = 1 << 20          # counters per work item; the key is (counter // CHUNK) % len(KEYS)
FULL_CHUNKS = 1          # chunks scanned for every window; later ones for S at W = 24 only
ROUND = 16               # chunks per round
MSG_TAG = b"comb-digit-edge:"
SEEDS = [bytes([0xC0 + k]) * 32 for k in range(4)]


@functools.lru_cache(None)
def rows_of(w):
    return -(-254 // w)


@functools.lru_cache(None)
def bias_of(w):
    return sum(1 << (w - 1 + w * i) for i in range(rows_of(w)))


def edge_values(w):
    half = 1 << (w - 1)
    return (-half, -half + 1, -1, 0, 1, half - 1)


def _count_below(n, w, i, f):
    """Number of y in [0, n) whose W-bit field i equals f."""
    lo, span = w * i, 1 << (w * i)
    full, rest = n >> (lo + w), n & ((1 << (lo + w)) - 1)
    return full * span + min(max(rest - f * span, 0), span)


def digit_count(w, i, v):
    """Number of scalars x in [0, L) whose digit i at window w is v."""
    f, b = v + (1 << (w - 1)), bias_of(w)
    return _count_below(b + L, w, i, f) - _count_below(b, w, i, f)


def all_targets():
    """(reachable, unreachable) lists of (kind, w, row, v)."""
    reach, unreach = [], []
    for kind, windows in (("S", S_WINDOWS), ("h", H_WINDOWS)):
        for w in windows:
            for i in range(rows_of(w)):
                for v in edge_values(w):
                    ok = digit_count(w, i, v) << -MIN_LOG2_PROB >= L
                    (reach if ok else unreach).append((kind, w, i, v))
    return reach, unreach


def digits(x, w):
    y = x + bias_of(w)
    return [((y >> (w * i)) & ((1 << w) - 1)) - (1 << (w - 1)) for i in range(rows_of(w))]


def key_material(k):
    seed = SEEDS[k]
    a, _ = E.secret_expand(seed)
    a %= L
    r = E.sha512_int(b"comb-digit-edge nonce", seed) % L
    return a, r


def message(c):
    return MSG_TAG + c.to_bytes(8, "little")


def _scan_chunk(args):
    """Lowest counter of the chunk for every target it hits: {(kind, w, row, v): counter}."""
    chunk, a, r, pre_bytes, full = args
    pre = hashlib.sha512(pre_bytes)
    b24 = bias_of(24)
    found = {}
    c0 = chunk * CHUNK
    step = 1 << 16
    wanted = {w: set(edge_values(w)) for w in set(S_WINDOWS + H_WINDOWS)}
    for base in range(c0, c0 + CHUNK, step):
        ys = []
        for c in range(base, base + step):
            hh = pre.copy()
            hh.update(MSG_TAG + c.to_bytes(8, "little"))
            h = int.from_bytes(hh.digest(), "little") % L
            s = (r + h * a) % L
            ys.append((s + b24).to_bytes(33, "little"))
            if full:
                for kind, x, windows in (("S", s, S_WINDOWS[1:]), ("h", h, H_WINDOWS)):
                    for w in windows:
                        for i, v in enumerate(digits(x, w)):
                            if v in wanted[w]:
                                found.setdefault((kind, w, i, v), c)
        # W = 24 fields are three whole bytes each: edge fields are those with (f + 1) mod 2^23 <= 2
        arr = np.frombuffer(b"".join(ys), np.uint8).reshape(step, 11, 3).astype(np.uint32)
        f = arr[:, :, 0] | (arr[:, :, 1] << 8) | (arr[:, :, 2] << 16)
        hit_t, hit_i = np.nonzero(((f + 1) & 0x7FFFFF) <= 2)
        for t, i in zip(hit_t.tolist(), hit_i.tolist()):
            found.setdefault(("S", 24, i, int(f[t, i]) - (1 << 23)), base + t)
    return found


def search(procs):
    reach, unreach = all_targets()
    keys = []
    for k in range(len(SEEDS)):
        a, r = key_material(k)
        A_enc, R_enc = E.encode(E.mul(a, E.B)), E.encode(E.mul(r, E.B))
        keys.append((a, r, A_enc, R_enc))
    best = {}
    chunk = 0
    with multiprocessing.Pool(procs) as pool:
        while not all(t in best for t in reach):
            jobs = []
            for ch in range(chunk, chunk + ROUND):
                a, r, A_enc, R_enc = keys[ch % len(keys)]
                jobs.append((ch, a, r, R_enc + A_enc, ch < FULL_CHUNKS * len(keys)))
            for found in pool.map(_scan_chunk, jobs, 1):
                for t, c in found.items():
                    if t not in best or c < best[t]:
                        best[t] = c
            chunk += ROUND
            print("chunks", chunk, "targets", sum(t in best for t in reach), "/", len(reach), flush=True)
    assert not any(t in best for t in unreach if digit_count(t[1], t[2], t[3]) == 0)
    return reach, unreach, best, keys, chunk


def load_sodium():
    import ctypes
    for cand in ("/opt/conda/lib/libsodium.so.23", "libsodium.so.23", "libsodium.so"):
        try:
            lib = ctypes.CDLL(cand)
        except OSError:
            continue
        lib.sodium_init()
        lib.sodium_version_string.restype = ctypes.c_char_p
        return lib
    raise SystemExit("libsodium not found")


def main():
    import ctypes
    sodium = load_sodium()
    assert sodium.sodium_version_string() == b"1.0.18", sodium.sodium_version_string()
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, len(os.sched_getaffinity(0)))
    reach, unreach, best, keys, chunks = search(procs)
    by_counter = {}
    for t in reach:
        by_counter.setdefault(best[t], []).append(t)
    items, labels = [], []
    for c in sorted(by_counter):
        a, r, A_enc, R_enc = keys[(c // CHUNK) % len(keys)]
        msg = message(c)
        h = E.sha512_int(R_enc, A_enc, msg) % L
        s = (r + h * a) % L
        for kind, w, i, v in by_counter[c]:
            assert digits(s if kind == "S" else h, w)[i] == v
        accept = len(items)
        items.append((R_enc + s.to_bytes(32, "little"), A_enc, msg))
        labels.append({"targets": [list(t) for t in by_counter[c]], "counter": c, "twin_of": None, "flip_bit": None})
        for bit in sorted({w * i if kind == "S" else 0 for kind, w, i, v in by_counter[c]}):
            items.append((R_enc + (s ^ (1 << bit)).to_bytes(32, "little"), A_enc, msg))
            labels.append({"targets": [], "counter": c, "twin_of": accept, "flip_bit": bit})
    sig = np.frombuffer(b"".join(i[0] for i in items), np.uint8).reshape(-1, 64)
    pk = np.frombuffer(b"".join(i[1] for i in items), np.uint8).reshape(-1, 32)
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(i[2]) for i in items])
    expect = np.array([sodium.crypto_sign_verify_detached(i[0], i[2], ctypes.c_ulonglong(len(i[2])), i[1]) == 0
                       for i in items], np.uint8)
    for lab, e in zip(labels, expect):
        assert bool(e) == (lab["twin_of"] is None), lab
    np.savez_compressed(os.path.join(HERE, "comb_digit_edge.npz"), sig=sig, pk=pk,
                        msgs=np.frombuffer(b"".join(i[2] for i in items), np.uint8), off=off, expect=expect)
    with open(os.path.join(HERE, "comb_digit_edge_labels.json"), "w") as f:
        json.dump({"libsodium": sodium.sodium_version_string().decode(), "trials": chunks * CHUNK,
                   "keys": [k[2].hex() for k in keys], "items": labels,
                   "unreachable": [list(t) for t in unreach], "expect": [int(x) for x in expect]}, f, indent=0)
    print("items:", len(items), "accepted:", int(expect.sum()), "targets:", len(reach), "unreachable:", len(unreach),
          "trials:", chunks * CHUNK)


if __name__ == "__main__":
    main()
