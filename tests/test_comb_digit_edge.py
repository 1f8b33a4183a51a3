"""tests/golden/comb_digit_edge.npz: valid signatures whose S or h has a digit on the comb's edges
(-2^(W-1), -2^(W-1)+1, -1, 0, 1, 2^(W-1)-1) in a chosen row -- the table entries and the
comb_set_entry / identity cases a random scalar reaches with probability 2^-W -- and their
one-bit-of-S twins.  Here: the labels are what they say and leave no reachable target out, the
verdicts are the oracle's, and the kernel arithmetic on the CPU (base window 16) agrees."""
import ctypes
import hashlib
import json
import os

import pytest

from conftest import GOLDEN, items_of, load_npz

L = 2**252 + 27742317777372353535851937790883648493
WINDOWS = {"S": (24, 16), "h": (10, 14, 16)}


def rows_of(w):
    return -(-254 // w)


def digits(x, w):
    """comb.h's recoding with plain integers: y = x + bias, digit_i = field_i(y) - 2^(W-1)."""
    half = 1 << (w - 1)
    y = x + sum(half << (w * i) for i in range(rows_of(w)))
    return [((y >> (w * i)) & (2 * half - 1)) - half for i in range(rows_of(w))]


def edge_values(w):
    half = 1 << (w - 1)
    return (-half, -half + 1, -1, 0, 1, half - 1)


def scalars_with_digit(w, i, v, limit=L):
    """How many x in [0, limit) have digit i = v at window w: y = x + bias runs over [bias, bias +
    limit), and field i of y equals f on 2^(w*i) consecutive values out of every 2^(w*(i+1))."""
    half = 1 << (w - 1)
    f, bias = v + half, sum(half << (w * k) for k in range(rows_of(w)))
    period, span = 1 << (w * (i + 1)), 1 << (w * i)

    def below(n):  # y in [0, n) with field i = f
        q, r = divmod(n, period)
        return q * span + min(max(r - f * span, 0), span)
    return below(bias + limit) - below(bias)


def enumerate_targets():
    """A target (kind, w, row, v) is reachable when a uniform scalar below L has that digit with
    probability at least 2^-26."""
    reach, unreach = set(), set()
    for kind, windows in WINDOWS.items():
        for w in windows:
            for i in range(rows_of(w)):
                for v in edge_values(w):
                    (reach if scalars_with_digit(w, i, v) * 2**26 >= L else unreach).add((kind, w, i, v))
    return reach, unreach


@pytest.fixture(scope="module")
def fixture():
    items = items_of(load_npz("comb_digit_edge.npz"))
    with open(os.path.join(GOLDEN, "comb_digit_edge_labels.json")) as f:
        labels = json.load(f)
    assert len(labels["items"]) == len(items) == len(labels["expect"])
    return items, labels


def scalars_of(item):
    sig, pk, msg, _ = item
    h = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
    return {"S": int.from_bytes(sig[32:], "little"), "h": h}


def test_scalar_count_formula_by_brute_force():
    """scalars_with_digit against counting, with a toy limit in place of L."""
    for toy in (1000, 4096, 5000):
        for w in (4, 5):
            all_digits = [digits(x, w) for x in range(toy)]
            for i in range(rows_of(w)):
                for v in edge_values(w):
                    assert scalars_with_digit(w, i, v, toy) == sum(d[i] == v for d in all_digits), (toy, w, i, v)


def test_labels_are_exact_and_complete(fixture):
    items, labels = fixture
    reach, unreach = enumerate_targets()
    seen = set()
    for idx, (item, lab) in enumerate(zip(items, labels["items"])):
        x = scalars_of(item)
        assert bool(labels["expect"][idx]) == item[3]
        if lab["twin_of"] is None:
            assert item[3] and lab["targets"], idx
            for kind, w, i, v in lab["targets"]:
                assert digits(x[kind], w)[i] == v, (idx, kind, w, i, v)
                seen.add((kind, w, i, v))
        else:  # one bit of S flipped, everything else the accept item's
            a = items[lab["twin_of"]]
            assert not item[3] and not lab["targets"]
            assert (item[0][:32], item[1], item[2]) == (a[0][:32], a[1], a[2])
            assert x["S"] ^ scalars_of(a)["S"] == 1 << lab["flip_bit"]
            tw = labels["items"][lab["twin_of"]]
            assert lab["flip_bit"] in {w * i if kind == "S" else 0 for kind, w, i, v in tw["targets"]}
    assert seen == reach
    assert {tuple(t) for t in labels["unreachable"]} == unreach
    # every S target has the twin at the low bit of its row, every h target one at bit 0
    twins = {(lab["twin_of"], lab["flip_bit"]) for lab in labels["items"] if lab["twin_of"] is not None}
    for idx, lab in enumerate(labels["items"]):
        for kind, w, i, v in lab["targets"]:
            assert (idx, w * i if kind == "S" else 0) in twins
    # what is out of reach: the top rows' negative and large digits
    assert all(i == rows_of(w) - 1 and v not in (0, 1) for _, w, i, v in unreach)
    assert os.path.getsize(os.path.join(GOLDEN, "comb_digit_edge.npz")) <= \
        max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "comb_digit_edge.npz")


def test_verdicts_are_the_oracles(fixture, oracle):
    items, labels = fixture
    assert labels["libsodium"] == "1.0.18"
    for idx, (sig, pk, msg, expect) in enumerate(items):
        assert (oracle.oracle_verify_detached(sig, msg, len(msg), pk) == 0) == expect, idx


def test_kernel_verify_on_cpu_over_the_digit_edges(fixture, hostcheck):
    """edv_host_verify (general path, base window 16): the W = 16 S targets read the last entry and
    the identity of every row of the host-built base table."""
    items, _ = fixture
    for idx, (sig, pk, msg, expect) in enumerate(items):
        assert (hostcheck.edv_host_verify(sig, pk, msg, ctypes.c_uint64(len(msg))) == 0) == expect, idx


@pytest.mark.parametrize("kw", [10, 14])
def test_kernel_comb_on_cpu_over_its_h_targets(fixture, hostcheck, kw):
    """The key-table path at W = 10 and 14 (comb_mul_set: comb_set_entry for row 0, the identity
    entry) over every item with an h target at that window, and its twins."""
    items, labels = fixture
    want = {idx for idx, lab in enumerate(labels["items"])
            if any(k == "h" and w == kw for k, w, _, _ in lab["targets"])}
    want |= {idx for idx, lab in enumerate(labels["items"]) if lab["twin_of"] in want}
    assert len(want) >= 2 * 80
    for idx in sorted(want, key=lambda k: (items[k][1], k)):  # key by key: the host build keeps the last key's table
        sig, pk, msg, expect = items[idx]
        got = hostcheck.edv_host_verify_comb_w(sig, pk, msg, ctypes.c_uint64(len(msg)), kw) == 0
        assert got == expect, (kw, idx)
