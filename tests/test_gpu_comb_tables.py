"""The comb tables the verify kernels read, entry by entry, and the comb's digit edges through
every verify path.

Every verify ends in [h](-A) + [S]B over the base point's table at window 24 (11 rows of 2^23
entries, built once per context by edv_comb_fill_kernel) and a key's table at windows 4 to 16.
Verdicts of random signatures read a vanishing part of them.  Here every entry is read back
(edv_comb_table_read) and checked by oracle/comb_table_check.c against one big-integer anchor per
row: all 11 x 2^23 base entries; every row of every key of a W = 10 store that has grown twice and
had slots re-registered both ways; first, middle and last slot of W = 14 and W = 16 stores.  Then
tests/golden/comb_digit_edge.npz -- signatures whose S or h has an edge digit in a chosen row, and
their one-bit twins -- must give its verdicts bit for bit through the general path, the batch comb
kernel, the three-wave small-batch kernel and both single-request paths."""
import json
import os
import time

import numpy as np
import pytest

import comb_table_util as T
import edwards as E
from conftest import GOLDEN, host_threads, load_npz

pytestmark = pytest.mark.gpu

BASE_W = 24
CHUNK = 1 << 20  # entries per read-back: 128 MiB


@pytest.fixture(scope="module")
def checker():
    return T.load_checker()


@pytest.fixture(scope="module")
def base_rows():
    return T.row_bases(E.B, BASE_W)


@pytest.fixture(scope="module")
def chunk_buf():
    return np.empty((CHUNK, 32), np.uint32)


def _threads_for(n_entries):
    return max(1, min(host_threads(), n_entries // 2048))


@pytest.mark.parametrize("row", range(11))
def test_base_table_row_entry_by_entry(gpu_engine, checker, base_rows, chunk_buf, row):
    """All 2^23 entries of one row of the shipped base table: entry 0 is 2^(24 row) B (doublings
    with Python integers), every entry its predecessor plus that, limbs canonical, pad zero, third
    field 2dxy; twice the last entry is the next row's base."""
    assert gpu_engine._lib.edv_base_window() == BASE_W and len(base_rows) == 11
    n = 1 << (BASE_W - 1)
    t_read = [0.0]

    def read(lo, cnt):
        t0 = time.perf_counter()
        out = gpu_engine.comb_table_read(-1, row, lo, cnt, out=chunk_buf[:cnt])
        t_read[0] += time.perf_counter() - t0
        return out
    t0 = time.perf_counter()
    bad, at, last = T.check_row(checker, read, n, base_rows[row], host_threads(), CHUNK)
    dt = time.perf_counter() - t0
    print("base row %d: %d entries in %.2f s (read-back %.2f s, %d threads)" % (row, n, dt, t_read[0], host_threads()))
    assert (bad, at) == (0, None)
    if row + 1 < len(base_rows):
        assert E.add(last, last) == base_rows[row + 1]


def _check_key(gpu_engine, checker, key_id, enc, w):
    """Every row of key_id's table against -A of the encoding that slot holds."""
    P = E.neg(E.decode(enc))
    n = 1 << (w - 1)
    return T.check_table(checker, lambda row, lo, cnt: gpu_engine.comb_table_read(key_id, row, lo, cnt), P, w,
                         _threads_for(n))


def _ordinary_keys():
    pk = load_npz("ed25519_valid.npz")["pk"]
    keys = list(dict.fromkeys(pk[i].tobytes() for i in range(len(pk))))
    assert len(keys) >= 220
    return keys


def _mixed_order_key():
    """A key A0 + T8 of the golden edge set that libsodium accepts a signature under."""
    d = load_npz("ed25519_edge.npz")
    with open(os.path.join(GOLDEN, "ed25519_edge_labels.json")) as f:
        labels = json.load(f)["labels"]
    i = next(k for k, lab in enumerate(labels) if lab.startswith("A=mixed-order-") and lab.endswith("k%8==0"))
    assert d["expect"][i]
    return d["pk"][i].tobytes()


N_KEYS_W10 = 130


class TestKeyStoreW10:
    @pytest.fixture(scope="class")
    def store(self, gpu_engine):
        """130 keys registered in slices of 40 (capacity 64 -> 128 -> 256, the store re-laid out
        twice), eleven scattered slots re-registered in one asynchronous call and eight consecutive
        ones synchronously: slot -> the encoding it now holds."""
        ordinary = _ordinary_keys()
        held = ordinary[:N_KEYS_W10]
        held[0] = E.encode(E.B)
        held[64] = _mixed_order_key()
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(10)
        try:
            for lo in range(0, N_KEYS_W10, 40):
                part = held[lo:lo + 40]
                assert gpu_engine.keys_add(np.frombuffer(b"".join(part), np.uint8).reshape(-1, 32)) == lo
            assert gpu_engine.keys_count() == N_KEYS_W10
            fresh = ordinary[N_KEYS_W10:]
            scattered = [1, 5, 31, 62, 63, 65, 100, 126, 128, 129, 90]  # 0, 64 and 127 stay: untouched neighbours
            for k, slot in enumerate(scattered):
                held[slot] = fresh[k]
            gpu_engine.keys_set_many_async(scattered, np.frombuffer(b"".join(held[s] for s in scattered),
                                                                    np.uint8).reshape(-1, 32))
            for k, slot in enumerate(range(40, 48)):
                held[slot] = fresh[20 + k]
            gpu_engine.keys_set(40, np.frombuffer(b"".join(held[40:48]), np.uint8).reshape(-1, 32))
            assert len(set(held)) == N_KEYS_W10
            yield held
        finally:
            gpu_engine.keys_reset()
            gpu_engine.keys_set_window(10)

    @pytest.mark.parametrize("part", range(4))
    def test_every_row_of_every_key(self, gpu_engine, checker, store, part):
        """All 26 rows x 512 entries of a quarter of the slots -- among all four: slots 0 (B's own
        encoding), 63, 64 (mixed order), 127, 128, every rewritten slot and every neighbour."""
        assert gpu_engine.keys_count() == N_KEYS_W10 and gpu_engine.keys_window == 10
        lo, hi = N_KEYS_W10 * part // 4, N_KEYS_W10 * (part + 1) // 4
        t0 = time.perf_counter()
        wrong = {}
        for slot in range(lo, hi):
            rows = _check_key(gpu_engine, checker, slot, store[slot], 10)
            if rows:
                wrong[slot] = rows
        print("W = 10 slots %d..%d: %.2f s" % (lo, hi - 1, time.perf_counter() - t0))
        assert wrong == {}

    def test_read_back_error_codes(self, gpu_engine, store):
        """EDV_EINVAL, the output untouched: a row at or beyond the table's rows, first + count one
        past the end, key_id = the key count, key_id < -1, and count = 0 (defined as an error, also
        at the end boundary)."""
        from plenum_amd._lib import EdVerifyError
        out = np.full((4, 32), 0xC3C3C3C3, np.uint32)
        cases = [(-1, 11, 0, 1), (-1, 1 << 30, 0, 1), (-1, 0, (1 << 23) - 3, 4), (-1, 10, 1 << 23, 1),
                 (-1, 0, (1 << 64) - 1, 2), (-1, 0, 1 << 23, 0), (-1, 0, 0, 0), (-2, 0, 0, 1),
                 (0, 26, 0, 1), (N_KEYS_W10 - 1, 25, 509, 4), (N_KEYS_W10 - 1, 25, 512, 1), (N_KEYS_W10, 0, 0, 1),
                 (1 << 40, 0, 0, 1), (0, 0, 512, 0)]
        for key_id, row, first, count in cases:
            with pytest.raises(EdVerifyError) as ex:
                gpu_engine.comb_table_read(key_id, row, first, count, out=out[:count])
            assert ex.value.code == -1, (key_id, row, first, count)
            assert (out == 0xC3C3C3C3).all(), (key_id, row, first, count)
        # the last entries of the last rows read fine, into exactly the words asked for
        got = gpu_engine.comb_table_read(-1, 10, (1 << 23) - 3, 3, out=out[:3])
        assert (got[:, 30:] == 0).all() and (out[3] == 0xC3C3C3C3).all()
        out[:] = 0xC3C3C3C3
        got = gpu_engine.comb_table_read(N_KEYS_W10 - 1, 25, 509, 3, out=out[:3])
        assert (got[:, 30:] == 0).all() and (out[3] == 0xC3C3C3C3).all()
        full = gpu_engine.comb_table_read(N_KEYS_W10 - 1, 25, 0, 512)
        assert np.array_equal(full[509:], got)


@pytest.mark.parametrize("w", [14, 16])
def test_key_tables_at_wide_windows(gpu_engine, checker, w):
    """W = 14 (19 rows x 8,192 entries, 256 fill lanes per row) and W = 16 (16 rows x 32,768, 1,024
    lanes): first, middle and last slot of a store of 65 keys registered as 40 + 25, so it has
    capacity 128 and was re-laid out once."""
    keys = _ordinary_keys()[150:215]
    keys[32] = E.encode(E.B)
    try:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(w)
        assert gpu_engine.keys_add(np.frombuffer(b"".join(keys[:40]), np.uint8).reshape(-1, 32)) == 0
        assert gpu_engine.keys_add(np.frombuffer(b"".join(keys[40:]), np.uint8).reshape(-1, 32)) == 40
        t0 = time.perf_counter()
        for slot in (0, 32, 64):
            assert _check_key(gpu_engine, checker, slot, keys[slot], w) == [], slot
        print("W = %d, three keys: %.2f s" % (w, time.perf_counter() - t0))
    finally:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(10)


# ---- scalars on the digit edges, through every verify path

@pytest.fixture(scope="module")
def edge():
    d = load_npz("comb_digit_edge.npz")
    with open(os.path.join(GOLDEN, "comb_digit_edge_labels.json")) as f:
        labels = json.load(f)
    keys = [bytes.fromhex(k) for k in labels["keys"]]
    kidx = np.array([keys.index(d["pk"][i].tobytes()) for i in range(len(d["expect"]))], np.uint32)
    out = dict(sig=d["sig"], pk=d["pk"], msgs=d["msgs"], off=d["off"], expect=d["expect"].astype(bool), kidx=kidx,
               keys=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32), labels=labels["items"])
    assert out["expect"].sum() * 2 < len(kidx) and out["expect"].sum() > 400
    return out


def _mismatch(got, edge):
    bad = np.flatnonzero(np.asarray(got, bool) != edge["expect"])
    return [(int(i), edge["labels"][i]) for i in bad[:5]]


def test_digit_edges_general_path(gpu_engine, edge):
    """verify_batch: the base comb at window 24 (the S targets at W = 24 read the last entry, the
    identity and their neighbours in every row)."""
    got = gpu_engine.verify_batch(edge["sig"], edge["pk"], edge["msgs"], edge["off"])
    assert _mismatch(got, edge) == []


@pytest.mark.parametrize("w", [10, 14, 16])
def test_digit_edges_keyed_paths(gpu_engine, edge, w):
    """verify_batch_keyed with the fixture's keys registered: the batch comb kernel (CombDigits,
    small_batch = 0) with the key sort off and on, and the three-wave kernel (comb_digit,
    comb_row_point; small_batch >= n)."""
    n = len(edge["kidx"])
    try:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(w)
        assert gpu_engine.keys_add(edge["keys"]) == 0
        for opts in (dict(small_batch=0, key_sort=0), dict(small_batch=0, key_sort=1), dict(small_batch=1024)):
            assert opts.get("small_batch", 0) == 0 or opts["small_batch"] >= n
            gpu_engine.set_options(**opts)
            got = gpu_engine.verify_batch_keyed(edge["sig"], edge["kidx"], edge["msgs"], edge["off"])
            assert _mismatch(got, edge) == [], (w, opts)
    finally:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(10)


@pytest.mark.parametrize("resident", [1, 0])
def test_digit_edges_single_request(gpu_engine, edge, resident):
    """verify_one for every accept item and every twin at W = 14, through the resident kernel and
    with it off (one launch of the small kernel per request): the S targets at W = 24 and the h
    targets at W = 14 are the ones these kernels' own digit code meets."""
    try:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(14)
        assert gpu_engine.keys_add(edge["keys"]) == 0
        gpu_engine.set_options(resident=resident)
        off = edge["off"]
        msgs = edge["msgs"].tobytes()
        got = [gpu_engine.verify_one_keyed(edge["sig"][i].tobytes(), int(edge["kidx"][i]),
                                           msgs[int(off[i]):int(off[i + 1])]) for i in range(len(edge["kidx"]))]
        assert _mismatch(got, edge) == []
    finally:
        gpu_engine.keys_reset()
        gpu_engine.keys_set_window(10)
