"""Helpers of the comb table tests (test_comb_table_check.py, test_gpu_comb_tables.py): the
table layout restated with Python integers, and the calls into oracle/comb_table_check.c.

Entry j of row i of the window-W table of a point P holds (j+1) * 2^(W*i) * P as 32 words:
(y+x, y-x, 2dxy) as three field elements of ten limbs at bits 0, 26, 51, 77, ... and 2 zero words."""
import ctypes
import os
import subprocess

import numpy as np

import edwards as E
from conftest import ROOT

LIMB_AT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
LIMB_BITS = [26, 25] * 5
ENTRY_WORDS = 32
HALF = E.inv(2)


def rows_of(w):
    return -(-254 // w)


def fe_limbs(v):
    return [(v >> s) & ((1 << b) - 1) for s, b in zip(LIMB_AT, LIMB_BITS)]


def fe_value(limbs):
    return sum(int(x) << s for x, s in zip(limbs, LIMB_AT))


def niels_entry(P):
    x, y = P
    return fe_limbs((y + x) % E.p) + fe_limbs((y - x) % E.p) + fe_limbs(2 * E.d * x * y % E.p) + [0, 0]


def entry_point(words):
    """The affine point an entry holds (its first two fields only)."""
    ypx, ymx = fe_value(words[0:10]), fe_value(words[10:20])
    return ((ypx - ymx) * HALF % E.p, (ypx + ymx) * HALF % E.p)


def row_bases(P, w, rows=None):
    """2^(w*i) * P for i < rows, by doublings."""
    out = []
    for _ in range(rows_of(w) if rows is None else rows):
        out.append(P)
        for _ in range(w):
            P = E.add(P, P)
    return out


def python_table(P, w, rows):
    """uint32[rows, 2^(w-1), 32]: the table of P's first `rows` rows, with Python integers only."""
    tab = np.zeros((rows, 1 << (w - 1), ENTRY_WORDS), np.uint32)
    for i, base in enumerate(row_bases(P, w, rows)):
        Q = base
        for j in range(1 << (w - 1)):
            tab[i, j] = niels_entry(Q)
            Q = E.add(Q, base)
    return tab


def load_checker():
    path = os.path.join(ROOT, "oracle", "_build", "libcomb_table_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "_build/libcomb_table_check.so"], cwd=os.path.join(ROOT, "oracle"))
    lib = ctypes.CDLL(path)
    lib.comb_table_check.restype = ctypes.c_int64
    lib.comb_table_check.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_uint64)]
    return lib


def _xy(P):
    return P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little")


def check_run(lib, entries, base, first, threads=1):
    """(bad entries, index of the first or None) of a run of entries whose first must hold `first`
    and whose every later entry must be its predecessor plus `base` (affine integer points)."""
    entries = np.ascontiguousarray(entries, np.uint32).reshape(-1, ENTRY_WORDS)
    first_bad = ctypes.c_uint64()
    bad = lib.comb_table_check(entries.ctypes.data, entries.shape[0], _xy(base), _xy(first), int(threads),
                               ctypes.byref(first_bad))
    assert bad >= 0, "comb_table_check: bad argument"
    return int(bad), (int(first_bad.value) if bad else None)


def check_row(lib, read, n_entries, base, threads=1, chunk=1 << 20):
    """Every entry of one row, read(first, count) -> uint32[count, 32] a chunk at a time: entry 0
    must hold `base`, and the last verified point of a chunk is carried over as the expected
    predecessor of the next.  Returns (bad entries, index of the first or None, the last entry's
    point -- meaningful when nothing is bad)."""
    bad_total, first_bad, expect = 0, None, base
    for lo in range(0, n_entries, chunk):
        cnt = min(chunk, n_entries - lo)
        part = read(lo, cnt)
        bad, at = check_run(lib, part, base, expect, threads)
        if bad and first_bad is None:
            first_bad = lo + at
        bad_total += bad
        last = entry_point(part.reshape(-1, ENTRY_WORDS)[-1])
        expect = E.add(last, base)
    return bad_total, first_bad, last


def check_table(lib, read_row, P, w, threads=1, chunk=1 << 20):
    """Every entry of every row of the window-w table of P, read_row(row, first, count) ->
    uint32[count, 32].  One big-integer anchor per row (2^(w*row) * P by doublings); twice the last
    entry of a row must be the next row's base.  Returns [(row, bad entries, first bad index)] of the
    rows with anything wrong (empty when the table is right)."""
    wrong = []
    bases = row_bases(P, w)
    for row, base in enumerate(bases):
        bad, at, last = check_row(lib, lambda lo, cnt: read_row(row, lo, cnt), 1 << (w - 1), base, threads, chunk)
        if bad == 0 and row + 1 < len(bases) and E.add(last, last) != bases[row + 1]:
            bad, at = 1, (1 << (w - 1)) - 1
        if bad:
            wrong.append((row, bad, at))
    return wrong
