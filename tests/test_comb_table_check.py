"""oracle/comb_table_check.c (the independent checker of comb table entries) against a table built
with Python integers and against deliberate corruptions of it, then over the whole tables that
csrc/comb.h's comb_rows and comb_fill_strided build on the CPU (libedv_hostcheck.so): every entry
of the tables of B and of one ordinary key at W = 4, 8, 10 and 16 (1, 4, 16 and 1024 fill lanes
per row)."""
import ctypes
import time

import numpy as np
import pytest

import comb_table_util as T
import edwards as E
from conftest import host_threads, load_npz


@pytest.fixture(scope="module")
def checker():
    return T.load_checker()


@pytest.fixture(scope="module")
def small_table():
    """Three rows of the W = 8 table of B, Python integers only."""
    tab = T.python_table(E.B, 8, 3)
    tab.setflags(write=False)
    return tab


def _check_rows(checker, tab, threads):
    out = []
    for row, base in enumerate(T.row_bases(E.B, 8, 3)):
        out.append(T.check_run(checker, tab[row], base, base, threads))
    return out


@pytest.mark.parametrize("threads", [1, 3, 16, 200])
def test_checker_passes_a_python_built_table(checker, small_table, threads):
    assert _check_rows(checker, small_table, threads) == [(0, None)] * 3
    # a run that starts inside a row, from the point its first entry must hold
    base = T.row_bases(E.B, 8, 2)[1]
    assert T.check_run(checker, small_table[1, 37:], base, E.mul(38, base), threads) == (0, None)
    assert T.check_run(checker, small_table[1, 37:38], base, E.mul(38, base), threads) == (0, None)


def _corruptions():
    p = E.p

    def flip_limb_bit(t, row, j):
        t[row, j, 13] ^= 1 << 7

    def flip_top_limb_bit(t, row, j):
        t[row, j, 9] ^= 1 << 24

    def swap_with_next(t, row, j):
        t[row, [j, j + 1]] = t[row, [j + 1, j]]

    def noncanonical_limb(t, row, j):  # value + p (below 2^256): the same field element, top limb over 25 bits
        v = T.fe_value(t[row, j, 0:10]) + p
        limbs = T.fe_limbs(v)
        limbs[9] = v >> 230
        t[row, j, 0:10] = limbs

    def noncanonical_low_limb(t, row, j):  # limb 0 + 2^26, limb 1 - 1: the same value, limb 0 out of range
        assert t[row, j, 11] > 0
        t[row, j, 10] += 1 << 26
        t[row, j, 11] -= 1

    def pad_word(t, row, j):
        t[row, j, 31] = 1

    def pad_word_30(t, row, j):
        t[row, j, 30] = 0x80000000

    def wrong_third_field(t, row, j):  # a canonical value, not 2dxy
        t[row, j, 20:30] = T.fe_limbs((T.fe_value(t[row, j, 20:30]) + 1) % p)

    def negated_point(t, row, j):  # -entry: a point of the curve with the right 2dxy sign flipped too
        x, y = T.entry_point(t[row, j])
        t[row, j] = T.niels_entry(((-x) % p, y))

    def other_multiple(t, row, j):  # a valid niels point, the wrong multiple
        t[row, j] = t[row, (j + 5) % t.shape[1]]

    # (corruption, bad entries it makes)
    return [(flip_limb_bit, 1), (flip_top_limb_bit, 1), (swap_with_next, 2), (noncanonical_limb, 1),
            (noncanonical_low_limb, 1), (pad_word, 1), (pad_word_30, 1), (wrong_third_field, 1), (negated_point, 1),
            (other_multiple, 1)]


@pytest.mark.parametrize("corrupt,n_bad", _corruptions(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_checker_reports_the_exact_index(checker, small_table, corrupt, n_bad):
    bases = T.row_bases(E.B, 8, 3)
    for row, j in ((0, 0), (0, 1), (1, 63), (2, 126), (1, 127), (2, 64)):
        if corrupt.__name__ == "swap_with_next" and j == 127:
            j = 126
        tab = small_table.copy()
        corrupt(tab, row, j)
        assert not np.array_equal(tab, small_table)
        for threads in (1, 2, 5, 128):
            got = [T.check_run(checker, tab[r], bases[r], bases[r], threads) for r in range(3)]
            for r in range(3):
                if r != row:
                    assert got[r] == (0, None), (row, j, threads)
            bad, at = got[row]
            assert at == j, (row, j, threads, got[row])
            assert bad == n_bad, (row, j, threads, got[row])


def test_checker_rejects_a_wrong_first_point_and_a_wrong_base(checker, small_table):
    bases = T.row_bases(E.B, 8, 3)
    # the run goes on from the point entry 0 should hold, so nothing after it matches either
    assert T.check_run(checker, small_table[1], bases[1], bases[0], 1) == (128, 0)
    bad, at = T.check_run(checker, small_table[1], bases[0], bases[1], 1)
    assert (bad, at) == (127, 1)


def test_checker_wants_values_below_p(checker):
    """A field whose limbs are all in range but whose value is p itself (0 + p): only the value
    check can see it."""
    ident = np.array(T.niels_entry(E.IDENTITY), np.uint32)
    assert T.check_run(checker, ident, E.B, E.IDENTITY) == (0, None)
    for field in (0, 1, 2):
        bad = ident.copy()
        v = T.fe_value(bad[10 * field:10 * field + 10]) + E.p
        if v >> 255:
            continue
        bad[10 * field:10 * field + 10] = T.fe_limbs(v)
        assert T.fe_value(bad[10 * field:10 * field + 10]) == v
        assert T.check_run(checker, bad, E.B, E.IDENTITY) == (1, 0), field


def _host_table(hostcheck, enc, negate, w):
    hostcheck.edv_host_comb_table.restype = ctypes.c_int64
    hostcheck.edv_host_comb_table.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    words = hostcheck.edv_host_comb_table(enc, negate, w, None)
    assert words == T.rows_of(w) * (1 << (w - 1)) * 32
    tab = np.full(words, 0xA5A5A5A5, np.uint32)
    assert hostcheck.edv_host_comb_table(enc, negate, w, tab.ctypes.data) == words
    return tab.reshape(T.rows_of(w), 1 << (w - 1), 32)


@pytest.mark.parametrize("w", [4, 8, 10, 16])
@pytest.mark.parametrize("which", ["B", "key"])
def test_host_built_tables_entry_by_entry(checker, hostcheck, which, w):
    """comb_rows + comb_fill_strided (the fill kernels' lane loop) on the CPU: every entry of every
    row, one big-integer anchor per row."""
    if which == "B":
        enc, negate, P = E.encode(E.B), 0, E.B
    else:  # the key store holds -A
        enc, negate = load_npz("ed25519_valid.npz")["pk"][3].tobytes(), 1
        P = E.neg(E.decode(enc))
    tab = _host_table(hostcheck, enc, negate, w)
    t0 = time.perf_counter()
    wrong = T.check_table(checker, lambda row, lo, cnt: tab[row, lo:lo + cnt], P, w, host_threads())
    dt = time.perf_counter() - t0
    print("W = %d: %d entries checked in %.3f s on %d threads (%.2f M entries/s)"
          % (w, tab.shape[0] * tab.shape[1], dt, host_threads(), tab.shape[0] * tab.shape[1] / dt / 1e6))
    assert wrong == []
    assert hostcheck.edv_host_comb_table(b"\x02" + b"\0" * 31, 0, w, None) == -1  # y = 2 is not on the curve
    assert hostcheck.edv_host_comb_table(enc, negate, 17, None) == -1
