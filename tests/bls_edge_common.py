"""Shared by tests/test_bls_edges.py (the CPU build of the device code) and
tests/test_gpu_bls_edges.py / tests/test_gpu_bls_fp.py (the kernels): the edge fixture
(tests/golden/bls_edge_vectors.json, written by tests/golden/gen_bls_edge_vectors.py) and the
operand tables of the Fp primitives with their expectations as plain Python integers.

The Fp entry points come in two builds with one signature: libedv_bls_probe.so
(tests/native/bls_fp_probe.hip, on the GPU) and libedv_hostcheck.so (csrc/host_check.cpp); a
failure on the first alone is the device's, on both the arithmetic's."""
import ctypes
import functools
import json
import os
import random
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bls_bn254_oracle as o  # noqa: E402

P = o.P
MONT = 1 << 256
MONT_INV = pow(MONT, P - 2, P)

# ------------------------------------------------------------------ the fixture
# the classes the issue names: the tests hold their own list, so a class dropped from the
# generator fails here
CASE_CLASSES = [
    "valid", "vk_generator", "vk_neg_generator", "wrong_message", "wrong_key",
    "dup_vk_sig_doubled", "dup_vk_sig_single", "cancel_vk_plus_third", "cancel_vk_sum_infinity", "single_vk_list",
    "multi25", "multi25_missing_signer", "neg_sig",
    "sig_x_plus_p", "sig_y_plus_p", "sig_x_equals_p", "sig_xonly_nonresidue", "sig_trailing_bytes",
    "vk_xa_plus_p", "vk_xb_plus_p", "vk_ya_plus_p", "vk_yb_plus_p", "vk_ab_swapped",
    "second_generator", "second_generator_key_on_first", "generator_zero", "generator_off_curve",
]
AGG_CLASSES = ["single", "doubled", "cancel_to_zero", "cancel_plus_third", "infinity_first", "infinity_last",
               "off_curve_first", "empty", "n25", "x_only"]
EDGE_SKS = [1, 2, 3, o.R - 1, o.R - 2, (o.R - 1) // 2, (o.R + 1) // 2, 1 << 31, 1 << 32, 1 << 63, 1 << 64, 1 << 128,
            1 << 253, (1 << 253) - 1, int("55" * 32, 16) % o.R, int("aa" * 32, 16) % o.R]
MSG_LENGTHS = [0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129, 183, 184, 1000]
CANDIDATES = [1, 2, 3, 7, 8, 15, 16]


class Fixture:
    def __init__(self):
        self.d = d = json.load(open(os.path.join(GOLDEN, "bls_edge_vectors.json")))
        self.points = [bytes.fromhex(p) for p in d["points"]]
        self.gens = [self.points[g["g"]] for g in d["generators"]]
        self.keys, self.signatures, self.cases, self.aggregates = d["keys"], d["signatures"], d["cases"], d["aggregates"]
        self.msgs = [bytes.fromhex(m["hex"]) for m in d["messages"]]
        self.messages = d["messages"]
        self.special = d["special_messages"]

    def pt(self, i):
        return self.points[i]

    def rows(self, idx):
        """Point indices -> uint8 [n, 128]."""
        return np.frombuffer(b"".join(self.points[i] for i in idx), np.uint8).reshape(-1, 128).copy()

    def check_conditions(self):
        """The conditions the generator asserts, again on the committed file."""
        d = self.d
        acc = sum(c["expect"] for c in self.cases)
        assert acc >= 40 and len(self.cases) - acc >= 40, (acc, len(self.cases))
        assert {c["class"] for c in self.cases} == set(CASE_CLASSES)
        assert {a["class"] for a in self.aggregates} == set(AGG_CLASSES)
        assert len(set(d["points"])) == len(d["points"]) and all(len(p) == 128 for p in self.points)
        sks = [int(k["sk"], 16) for k in self.keys]
        assert sks[:len(EDGE_SKS)] == EDGE_SKS
        assert sum(1 for k in self.keys if not k["in_contract"]) == 3
        assert sorted(s for s, k in zip(sks, self.keys) if not k["in_contract"]) == [0, o.R, o.R + 1]
        assert all("outside the header's sk < r contract" in k["label"] for k in self.keys if not k["in_contract"])
        assert all(0 < s < o.R for s, k in zip(sks, self.keys) if k["in_contract"])
        assert [len(m) for m in self.msgs[:len(MSG_LENGTHS)]] == MSG_LENGTHS
        n = len(MSG_LENGTHS)
        assert [m["q"] for m in self.messages[n:n + 7]] == list(range(7))
        assert [m["candidate"] for m in self.messages[n + 7:n + 14]] == CANDIDATES
        assert self.messages[self.special["candidate_15"]]["candidate"] == 15
        assert self.messages[self.special["candidate_16"]]["candidate"] == 16
        assert self.messages[self.special["redo"]]["candidate"] > 16
        # a generator with x.a = p exactly decodes to infinity; with x.a = 0 it is that point
        assert self.gens[5][:32] == P.to_bytes(32, "big") and self.gens[4] == bytes(32) + self.gens[5][32:]
        over = {g: [self.points[k["vk"]] for k in self.keys if k["gen"] == g] for g in (4, 5)}
        assert over[5] == [bytes(128)] * 2 and over[4][0] == self.gens[4] and over[4][1] not in (self.gens[4], bytes(128))
        for c in self.cases:  # no expectation without the fields the generator derives it from
            assert set(c) == {"name", "class", "sig", "msg", "vks", "gen", "expect"} and isinstance(c["expect"], bool)
        for k, key in enumerate(self.keys[:20]):  # every edge key and every message in an accepting check
            assert any(c["expect"] and c["vks"] == [key["vk"]] for c in self.cases), k
        for m in range(len(self.msgs)):
            assert any(c["expect"] and c["msg"] == m for c in self.cases), m


@functools.lru_cache(None)
def fixture():
    return Fixture()


def main_cases(fx):
    """The cases over the reference generator (one launch takes one generator)."""
    return [c for c in fx.cases if c["gen"] == 0]


def pack_cases(fx, cases, junk_msg=b"", junk_vk=0):
    """(sig[n,128], msgs, msg_off, vk[m,128], vk_off, want) of a batch laid out with vk_off; junk
    prefixes make msg_off[0] and vk_off[0] nonzero."""
    buf = junk_msg + b"".join(fx.msgs[c["msg"]] for c in cases)
    off = np.cumsum([len(junk_msg)] + [len(fx.msgs[c["msg"]]) for c in cases]).astype(np.uint64)
    vk_idx = [i for c in cases for i in c["vks"]]
    vk_off = np.cumsum([junk_vk] + [len(c["vks"]) for c in cases]).astype(np.uint64)
    vks = np.zeros((junk_vk + len(vk_idx), 128), np.uint8)
    vks[:junk_vk] = 0xA5
    if vk_idx:
        vks[junk_vk:] = fx.rows(vk_idx)
    return (fx.rows([c["sig"] for c in cases]), np.frombuffer(buf, np.uint8), off, vks, vk_off,
            np.array([c["expect"] for c in cases], bool))


# ------------------------------------------------------------------ Fp operand tables
def limbs(values):
    """ints -> uint32 [n, 8] little-endian limbs."""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), "<u4").reshape(-1, 8).copy()


def ints(a):
    """uint32 [n, 8] -> ints."""
    raw = np.ascontiguousarray(a, "<u4").tobytes()
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]


@functools.lru_cache(None)
def boundary():
    """About 40 in-contract values (below p) where carries, borrows and reductions turn."""
    rm = MONT % P
    v = [0, 1, 2, 3, P - 1, P - 2, P - 3, (P - 1) // 2, (P + 1) // 2, (1 << 31), (1 << 32) - 1, 1 << 32, (1 << 63),
         (1 << 64) - 1, 1 << 64, 1 << 128, (1 << 128) - 1, 1 << 253, (1 << 253) - 1, rm, rm * rm % P, P - rm,
         (rm + 1) % P, MONT_INV]
    v += [0xffffffff << (32 * k) for k in range(8)]        # each single limb all ones
    v += [P - (1 << (32 * k)) for k in range(8)]           # p with one limb lowered by 1
    out = []
    for x in v:
        if 0 <= x < P and x not in out:  # in contract only (the top limb all ones is past p)
            out.append(x)
    assert 36 <= len(out) <= 44
    return out


@functools.lru_cache(None)
def pair_table():
    """All ordered pairs of the boundary set, then 4096 random pairs."""
    b = boundary()
    rng = random.Random(254)
    pairs = [(x, y) for x in b for y in b] + [(rng.randrange(P), rng.randrange(P)) for _ in range(4096)]
    return pairs


FP_OPS = {"add": 0, "sub": 1, "neg": 2, "dbl": 3, "mul": 4, "inv": 5}
FP_WANT = {
    "add": lambda a, b: (a + b) % P,
    "sub": lambda a, b: (a - b) % P,
    "neg": lambda a, b: -a % P,
    "dbl": lambda a, b: 2 * a % P,
    "mul": lambda a, b: a * b * MONT_INV % P,
    "inv": lambda a, b: pow(a, P - 2, P),
}


def check_fp(fn, name):
    """fn(op, a, b, n, out) over the pair table against Python integers."""
    pairs = pair_table()
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    out = np.full_like(a, 0xdeadbeef)
    rc = fn(FP_OPS[name], a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_uint64(len(pairs)), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    want = FP_WANT[name]
    bad = [(hex(x), hex(y), hex(g)) for (x, y), g in zip(pairs, ints(out)) if g != want(x, y)]
    assert not bad, (name, len(bad), bad[:3])


class Layout:
    def __init__(self, fn):
        v = (ctypes.c_uint32 * 7)()
        fn(v)
        self.op_words, self.max_terms, self.nop, self.mul, self.inv, self.zchk, self.lin = list(v)


class ExecTable:
    """Program operations over one read-only slot table (slot 0 holds zero: the fields an operation
    does not use name it, as the generated program's do), with what each must produce."""

    def __init__(self, lay):
        self.lay = lay
        self.slot_of = {0: 0}
        self.slots = [0]
        self.ops = []      # words
        self.want = []     # (wrote, flag, value or None, note)

    def slot(self, v):
        assert 0 <= v < P
        if v not in self.slot_of:
            self.slot_of[v] = len(self.slots)
            self.slots.append(v)
        return self.slot_of[v]

    def _emit(self, kind, n_a, n_b, mask, terms, want, note):
        lay = self.lay
        halves = [0] + [self.slot(t) for t in terms]
        halves += [0] * (2 * (lay.op_words - 1) - len(halves))
        w = [kind | (n_a << 4) | (n_b << 8) | (mask << 12)]
        w += [halves[2 * i] | (halves[2 * i + 1] << 16) for i in range(lay.op_words - 1)]
        self.ops.append(w)
        self.want.append(want + (note,))

    def lin(self, terms, mask):
        s = sum(-t if (mask >> i) & 1 else t for i, t in enumerate(terms)) % P
        self._emit(self.lay.lin, len(terms), 0, mask, list(terms) + [0] * (self.lay.max_terms - len(terms)),
                   (1, 0, s), ("lin", len(terms), mask))

    def mul(self, ta, tb, mask):
        """(signed sum of ta) * (signed sum of tb) / 2^256; mask bits 0-1 negate ta, 2-3 tb."""
        sa = sum(-t if (mask >> i) & 1 else t for i, t in enumerate(ta)) % P
        sb = sum(-t if (mask >> (2 + i)) & 1 else t for i, t in enumerate(tb)) % P
        terms = list(ta) + [0] * (2 - len(ta)) + list(tb) + [0] * (2 - len(tb))
        self._emit(self.lay.mul, len(ta), len(tb), mask, terms, (1, 0, sa * sb * MONT_INV % P),
                   ("mul", tuple(map(hex, ta)), tuple(map(hex, tb)), mask))

    def inv(self, s):
        self._emit(self.lay.inv, 1, 0, 0, [s], (1, 0, pow(s, P - 2, P) * MONT * MONT % P), ("inv", hex(s)))

    def zchk(self, s, t):
        self._emit(self.lay.zchk, 1, 1, 0, [s, t], (0, int(s == 0 and t == 0), None), ("zchk", hex(s), hex(t)))

    def run(self, fn):
        n = len(self.ops)
        assert len(self.slots) < 65536
        ops = np.asarray(self.ops, np.uint32).reshape(n, self.lay.op_words)
        slots = limbs(self.slots)
        out = np.full((n, 8), 0xdeadbeef, np.uint32)
        wrote = np.full(n, 7, np.uint8)
        flag = np.full(n, 7, np.uint32)
        vp = ctypes.c_void_p
        rc = fn(ops.ctypes.data_as(vp), ctypes.c_uint64(n), slots.ctypes.data_as(vp), ctypes.c_uint64(len(self.slots)),
                out.ctypes.data_as(vp), wrote.ctypes.data_as(vp), flag.ctypes.data_as(vp))
        assert rc == 0, rc
        bad = []
        for (w, f, v, note), gw, gf, gv in zip(self.want, wrote.tolist(), flag.tolist(), ints(out)):
            if gw != w or gf != f or (v is not None and gv != v) or (v is None and gv != 0):
                bad.append((note, (gw, gf, hex(gv)), (w, f, None if v is None else hex(v))))
        assert not bad, (len(bad), bad[:3])
        return n


def sum_sets(n, rng):
    """The operand sets of an n-term sum: all p - 1, all 0, pairs x, p - x, and sets whose plain sum
    is exactly p, 2p, 4p, 8p and each of those less one (n = 12 of p - 1 is 12p - 12)."""
    sets = [[P - 1] * n, [0] * n]
    x = rng.randrange(1, P)
    sets.append([x if i % 2 == 0 else P - x for i in range(n)])
    sets.append([1 if i % 2 == 0 else P - 1 for i in range(n)])
    for k in (1, 2, 4, 8):
        for t in (k * P, k * P - 1):
            base = t // n
            vals = [base] * n
            for i in range(0, n - 1, 2):  # spread: the sum stays
                d = rng.randrange(0, min(vals[i], P - 1 - vals[i + 1]) + 1) if vals[i + 1] <= P - 1 else 0
                vals[i] -= d
                vals[i + 1] += d
            vals[-1] += t - sum(vals)
            if all(0 <= v < P for v in vals):
                assert sum(vals) == t
                sets.append(vals)
    return sets


def build_lin_table(lay):
    """Every term count 1..kMaxTerms with every sign mask over sum_sets."""
    rng = random.Random(12)
    t = ExecTable(lay)
    reached = set()
    for n in range(1, lay.max_terms + 1):
        for vals in sum_sets(n, rng):
            reached.add(sum(vals))
            for mask in range(1 << n):
                t.lin(vals, mask)
    for k in (1, 2, 4, 8):
        assert k * P in reached and k * P - 1 in reached
    assert 12 * P - 12 in reached
    return t


def build_mul_inv_zchk_table(lay):
    rng = random.Random(13)
    b = boundary()
    t = ExecTable(lay)
    for x in b:
        for y in b:
            t.mul([x], [y], 0)
    for x in b[::3]:
        for y in b[::3]:
            for mask in (1, 4, 5):
                t.mul([x], [y], mask)
    for x in b:  # two-term sums on both sides: x + (p - x) = 0 mod p, x - x, (p - 1) + (p - 1), ...
        for mask in range(16):
            t.mul([x, (P - x) % P], [b[(b.index(x) + 5) % len(b)], P - 1], mask)
            t.mul([P - 1, P - 1], [x, x], mask)
    for _ in range(1024):
        q = [rng.randrange(P) for _ in range(4)]
        t.mul(q[:2], q[2:], rng.randrange(16))
    for x in b + [rng.randrange(P) for _ in range(256)]:
        t.inv(x)
    nz = [1, P - 1, 1 << 32, 1 << 224, 0xffffffff]
    t.zchk(0, 0)
    for x in nz:
        t.zchk(0, x)
        t.zchk(x, 0)
        t.zchk(x, nz[0])
    return t
