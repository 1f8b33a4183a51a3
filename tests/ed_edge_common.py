"""Tables and references for the Ed25519 arithmetic probes: tests/test_gpu_ed_probe.py runs them
through libedv_ed_probe.so on the device (tests/native/ed_probe.hip), tests/test_ed_edges.py through
the CPU twins edv_host_ed_* of libedv_hostcheck.so (the same calls, csrc/ed_probe_ops.h, with the
EDV_BOUND_CHECK assertions).  Every expectation is computed here from Python integers and
tests/golden/edwards.py; every comparison is exact.

A Probe wraps one of the two libraries.  The check_* functions build a table, run it, compare and
return the number of items they ran."""
import ctypes
import functools
import hashlib
import random

import numpy as np

import edwards as E
import test_fe_lanes_model as M

p, L, d = E.p, E.L, E.d
POS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
WID = [26, 25] * 5
TWO_P = [2 ** 27 - 38] + [2 ** 26 - 2 if k % 2 else 2 ** 27 - 2 for k in range(1, 10)]
FOUR_P = [2 * v for v in TWO_P]
# the operand classes of fe25519.h (EDV_IS_C / EDV_IS_L / EDV_IS_W), as inclusive limb maxima
C_MAX = [(1 << 26) - 1 if k % 2 == 0 else (1 << 25) + (1 << 18) for k in range(10)]
L_MAX = [3 << 26 if k % 2 == 0 else (3 << 25) + (1 << 18) for k in range(10)]
W_MAX = [5 << 26 if k % 2 == 0 else (5 << 25) + (1 << 18) for k in range(10)]
ANY_MAX = [2 ** 31 - 1] * 10  # fe_carry: "any class up to 2^31 per limb"

LANE_OPS = ["fe_mul", "fe_sq", "fe_sqn", "fe_add", "fe_sub", "fe_sub4", "fe_neg", "fe_carry", "fe_tobytes",
            "fe_frombytes", "fe_invert", "fe_pow22523", "fe_iszero", "fe_isnegative", "fe_cmov",
            "sc_reduce", "sc_is_canonical", "sc_muladd", "recode16", "comb10", "comb14", "comb16", "comb_base",
            "ge_frombytes", "has_small_order", "is_canonical_point", "ge_add", "ge_sub", "ge_madd", "ge_msub",
            "ge_add_signed", "p2_dbl", "p3_dbl", "comb_set_entry", "ge_tobytes", "sig_slot"]
OP = {name: i for i, name in enumerate(LANE_OPS)}
WAVE_OPS = ["dist_sq", "dist_mul", "dist_sqn", "cols_carry", "dist_round", "r_decode", "tree_sum"]
WOP = {name: i for i, name in enumerate(WAVE_OPS)}

FIELD_OPS = LANE_OPS[:15]
SCALAR_OPS = ["sc_reduce", "sc_is_canonical", "sc_muladd"]
RECODE_OPS = ["recode16", "comb10", "comb14", "comb16", "comb_base"]
GROUP_OPS = ["ge_add", "ge_sub", "ge_madd", "ge_msub", "ge_add_signed", "p2_dbl", "p3_dbl", "comb_set_entry",
             "ge_tobytes"]

_P = ctypes.c_void_p
_U64 = ctypes.c_uint64


class Probe:
    """The entry points of one library: prefix "edprobe" (the device) or "edv_host_ed" (the CPU twins,
    which have no wave forms)."""

    def __init__(self, lib, prefix, wave):
        self.lane_fn = getattr(lib, prefix + "_lane")
        self.lane_io = getattr(lib, prefix + "_lane_io")
        self.hash_fn = getattr(lib, prefix + "_hash")
        self.base_w = getattr(lib, prefix + "_base_w")()
        self.wave_fn = getattr(lib, prefix + "_wave") if wave else None
        self.wave_io = getattr(lib, prefix + "_wave_io") if wave else None
        for f in (self.lane_fn, self.lane_io, self.hash_fn, self.wave_fn, self.wave_io):
            if f is not None:
                f.restype = ctypes.c_int

    def lane(self, name, rows):
        """rows: n items of the op's input words -> an (n, out words) uint32 array"""
        io = (ctypes.c_int * 2)()
        assert self.lane_io(OP[name], io) == 0
        a = np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(len(rows), -1))
        assert a.shape[1] == io[0], (name, a.shape, io[0])
        out = np.zeros((len(rows), io[1]), np.uint32)
        r = self.lane_fn(OP[name], _P(a.ctypes.data), _U64(len(rows)), _P(out.ctypes.data))
        assert r == 0, (name, r)
        return out

    def wave(self, name, rows, aux=0):
        io = (ctypes.c_int * 2)()
        assert self.wave_io(WOP[name], io) == 0
        a = np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(len(rows), -1))
        assert a.shape[1] == io[0], (name, a.shape, io[0])
        out = np.zeros((len(rows), io[1]), np.uint32)
        r = self.wave_fn(WOP[name], _P(a.ctypes.data), ctypes.c_uint32(aux), _U64(len(rows)), _P(out.ctypes.data))
        assert r == 0, (name, r)
        return out

    def hash(self, form, sig, pk, buf, start, mlen):
        n = len(start)
        s = np.ascontiguousarray(np.frombuffer(b"".join(sig), np.uint8))
        k = np.ascontiguousarray(np.frombuffer(b"".join(pk), np.uint8))
        b = np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8))
        st, ml = np.array(start, np.uint64), np.array(mlen, np.uint64)
        h, ok = np.zeros((n, 8), np.uint32), np.zeros(n, np.uint8)
        r = self.hash_fn(form, _P(s.ctypes.data), _P(k.ctypes.data), _P(b.ctypes.data), _U64(len(b)),
                         _P(st.ctypes.data), _P(ml.ctypes.data), _U64(n), _P(h.ctypes.data), _P(ok.ctypes.data))
        assert r == 0, (form, r)
        return [int.from_bytes(h[i].tobytes(), "little") for i in range(n)], [bool(v) for v in ok]


# ---- words and limbs
def val(limbs):
    """the integer a limb vector stands for (not reduced)"""
    return sum(int(v) << s for v, s in zip(limbs, POS))


def canon_limbs(x):
    """x < 2^255 in limbs of their own widths"""
    assert 0 <= x < 2 ** 255
    return [(x >> POS[k]) & ((1 << WID[k]) - 1) for k in range(10)]


def limb_form(x, cls_max):
    """x as limbs inside a class, every limb taken as large as the class lets it be from the top
    (for x < 2^255 not the canonical split); None where the class cannot hold x that way"""
    out = [0] * 10
    for k in range(9, -1, -1):
        out[k] = min(cls_max[k], x >> POS[k])
        x -= out[k] << POS[k]
    return out if x == 0 else None


def words8(x):
    return [(x >> (32 * k)) & 0xffffffff for k in range(8)]


def words16(x):
    return [(x >> (32 * k)) & 0xffffffff for k in range(16)]


def int_of(words):
    return sum(int(w) << (32 * k) for k, w in enumerate(words))


def signed(w):
    w = int(w)
    return w - (1 << 32) if w >> 31 else w


def in_class(limbs, cls_max):
    return all(int(v) <= m for v, m in zip(limbs, cls_max))


SPECIAL_VALUES = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 ** 255 - 1, 2 ** 255 + 18]


def special_forms(cls_max, values=SPECIAL_VALUES):
    """the limb forms, inside a class, of the values around 0, p, 2p and 2^255: the canonical split
    where the value is below 2^255, and the top-heavy form of limb_form where the class holds it"""
    out = []
    for x in values:
        forms = []
        if x < 2 ** 255:
            forms.append(canon_limbs(x))
        f = limb_form(x, cls_max)
        if f is not None and f not in forms:
            forms.append(f)
        assert all(val(f) == x and in_class(f, cls_max) for f in forms)
        out += forms
    return out


def edge_patterns(cls_max):
    """every limb at its class maximum, and at maximum - 1; each single limb at maximum with the
    rest 0; even limbs at maximum with odd limbs 0, and the reverse; the special values' forms"""
    out = [list(cls_max), [m - 1 for m in cls_max]]
    out += [[cls_max[k] if k == j else 0 for k in range(10)] for j in range(10)]
    out += [[cls_max[k] if k % 2 == 0 else 0 for k in range(10)], [cls_max[k] if k % 2 else 0 for k in range(10)]]
    return out + special_forms(cls_max)


def random_patterns(cls_max, rng, n):
    """within class; a third of them with every limb in the top 16 values of its class"""
    return [[m - rng.randrange(16) if t % 3 == 0 else rng.randrange(m + 1) for m in cls_max] for t in range(n)]


N_RANDOM = 4096


# ---- field
def _pairs(fa, fb, ra, rb):
    return [(a, b) for a in fa for b in fb] + list(zip(ra, rb))


def check_field(pr, name):
    rng = random.Random(1000 + OP[name])
    if name == "fe_mul":  # f in W, g in L
        items = _pairs(edge_patterns(W_MAX), edge_patterns(L_MAX), random_patterns(W_MAX, rng, N_RANDOM),
                       random_patterns(L_MAX, rng, N_RANDOM))
        out = pr.lane(name, [a + b for a, b in items])
        for (a, b), o in zip(items, out):
            assert val(o) % p == val(a) * val(b) % p, (name, a, b, list(o))
            assert in_class(o, C_MAX), (name, a, b, list(o))
    elif name in ("fe_sq", "fe_invert", "fe_pow22523"):
        # fe_sq: f in L; the two exponentiations: the class C their callers pass (and 0 -> 0)
        cls = L_MAX if name == "fe_sq" else C_MAX
        items = edge_patterns(cls) + random_patterns(cls, rng, N_RANDOM)
        e = {"fe_sq": 2, "fe_invert": p - 2, "fe_pow22523": (p - 5) // 8}[name]
        out = pr.lane(name, items)
        for a, o in zip(items, out):
            assert val(o) % p == pow(val(a), e, p), (name, a, list(o))
            assert in_class(o, C_MAX), (name, a, list(o))
        assert any(val(a) % p == 0 for a in items)  # fe_invert(0) = 0 is in the table
    elif name == "fe_sqn":
        edge = edge_patterns(L_MAX)
        items = [(a, n) for a in edge for n in (1, 2, 3)] + [(a, 100) for a in edge[:4]]
        items += [(a, rng.randrange(1, 21)) for a in random_patterns(L_MAX, rng, N_RANDOM)]
        out = pr.lane(name, [a + [n] for a, n in items])
        for (a, n), o in zip(items, out):
            assert val(o) % p == pow(val(a), 2 ** n, p), (name, a, n, list(o))
            assert in_class(o, C_MAX), (name, a, n, list(o))
    elif name in ("fe_add", "fe_sub", "fe_sub4"):
        # the subtrahend classes: fe_sub g in C, fe_sub4 g in L; f up to W (no limb leaves 32 bits)
        gcls = L_MAX if name == "fe_sub4" else C_MAX
        items = _pairs(edge_patterns(W_MAX), edge_patterns(gcls), random_patterns(W_MAX, rng, N_RANDOM),
                       random_patterns(gcls, rng, N_RANDOM))
        out = pr.lane(name, [a + b for a, b in items])
        bias = {"fe_add": None, "fe_sub": TWO_P, "fe_sub4": FOUR_P}[name]
        for (a, b), o in zip(items, out):
            want = [x + y for x, y in zip(a, b)] if bias is None else [x + m - y for x, y, m in zip(a, b, bias)]
            assert list(map(int, o)) == want, (name, a, b)
            assert val(o) % p == (val(a) + val(b) if bias is None else val(a) - val(b)) % p
    elif name == "fe_neg":
        items = edge_patterns(C_MAX) + random_patterns(C_MAX, rng, N_RANDOM)
        out = pr.lane(name, items)
        for a, o in zip(items, out):
            assert list(map(int, o)) == [m - x for x, m in zip(a, TWO_P)] and val(o) % p == -val(a) % p, (name, a)
    elif name == "fe_carry":
        items = []
        for cls in (C_MAX, L_MAX, W_MAX, ANY_MAX):
            items += edge_patterns(cls) + random_patterns(cls, rng, N_RANDOM // 4)
        out = pr.lane(name, items)
        for a, o in zip(items, out):
            assert val(o) % p == val(a) % p and in_class(o, C_MAX), (name, a, list(o))
    elif name in ("fe_tobytes", "fe_iszero", "fe_isnegative"):
        # fe_canon's inputs: the classes its callers pass (C: a coordinate; L: a sum or difference of
        # two), and every form of the values of [0, 2p + 18] at its ends and around p, 2p and 2^255
        more = SPECIAL_VALUES + [2, 19, p - 2, p + 2, 2 * p + 1, 2 * p + 18, 2 ** 255, 2 ** 255 + 19]
        items = []
        for cls in (C_MAX, L_MAX):
            items += edge_patterns(cls) + special_forms(cls, more) + random_patterns(cls, rng, N_RANDOM // 2)
        assert any(val(a) == 2 * p + 18 for a in items)
        out = pr.lane(name, items)
        for a, o in zip(items, out):
            v = val(a) % p
            want = words8(v) if name == "fe_tobytes" else [int(v == 0)] if name == "fe_iszero" else [v & 1]
            assert list(map(int, o)) == want, (name, a, list(o))
    elif name == "fe_frombytes":
        xs = [0, 1, p - 1, p, p + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1, 2 ** 255 + 18, 2 ** 256 - 19]
        xs += [1 << b for b in range(256)] + [(2 ** 256 - 1) ^ (1 << b) for b in range(256)]
        xs += [rng.getrandbits(256) for _ in range(N_RANDOM)]
        out = pr.lane(name, [words8(x) for x in xs])
        for x, o in zip(xs, out):
            assert list(map(int, o)) == canon_limbs(x & (2 ** 255 - 1)), (name, hex(x))
        items = xs
    else:
        assert name == "fe_cmov"
        items = [(a, b, t & 1) for t, (a, b) in enumerate(zip(random_patterns(W_MAX, rng, 512),
                                                              random_patterns(W_MAX, rng, 512)))]
        items += [(list(W_MAX), [0] * 10, 1), (list(W_MAX), [0] * 10, 0), ([0] * 10, list(ANY_MAX), 1),
                  ([0] * 10, list(ANY_MAX), 0)]
        out = pr.lane(name, [a + b + [c] for a, b, c in items])
        for (a, b, c), o in zip(items, out):
            assert list(map(int, o)) == (a if c else b), (name, a, b, c)
    return len(items)


# ---- scalars
def sc_reduce_inputs():
    rng = random.Random(6)
    xs = [0, 1, L - 1, L, L + 1, 2 * L, 2 ** 512 - 1, 2 ** 512 - 1 - L, 2 ** 252, 2 ** 253 - 1,
          (2 ** 256 - 1) * L % 2 ** 512]  # the specials of test_kernel_sc_reduce_and_canonical
    for k in (1, 2, 15, 16, 17, 2 ** 512 // L):
        xs += [k * L - 1, k * L, k * L + 1]
    for i in range(25):
        xs += [x for x in (2 ** (21 * i) - 1, 2 ** (21 * i), 2 ** (21 * i) + 1) if 0 <= x < 2 ** 512]
    hi = sum((2 ** 21 - 1) << (21 * i) for i in range(12, 25)) % 2 ** 512  # limbs 12..24 all ones, 0..11 zero
    lo = sum((2 ** 21 - 1) << (21 * i) for i in range(12))                 # the reverse
    xs += [hi, lo, hi | lo]
    assert all(0 <= x < 2 ** 512 for x in xs)
    return xs + [rng.getrandbits(512) for _ in range(N_RANDOM)]


def check_scalar(pr, name):
    rng = random.Random(16)
    if name == "sc_reduce":
        xs = sc_reduce_inputs()
        out = pr.lane(name, [words16(x) for x in xs])
        for x, o in zip(xs, out):
            assert int_of(o) == x % L, (name, hex(x), hex(int_of(o)))
        return len(xs)
    if name == "sc_is_canonical":
        xs = [0, 1, L - 1, L, L + 1, 2 ** 256 - 1, 2 ** 255, L | 2 ** 255, 2 ** 252, 2 ** 252 - 1, 2 * L]
        xs += [L ^ (1 << b) for b in range(256)] + [(L - 1) ^ (1 << b) for b in range(256)]
        xs += [L + (k << (32 * w)) for w in range(8) for k in (-1, 1) if 0 <= L + (k << (32 * w)) < 2 ** 256]
        xs += [rng.getrandbits(256) for _ in range(1000)] + [rng.randrange(L) for _ in range(1000)]
        out = pr.lane(name, [words8(x) for x in xs])
        for x, o in zip(xs, out):
            assert int(o[0]) == int(x < L), (name, hex(x))
        return len(xs)
    assert name == "sc_muladd"  # inside its contract a b + c < 2^512
    ab = [0, 1, L - 1, L, 2 ** 252, 2 ** 254 + 2 ** 253 - 8]
    items = [(a, b, c) for a in ab for b in ab for c in (0, L - 1, 2 ** 256 - 1)]
    items += [(rng.getrandbits(255), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(1000)]
    assert all(a * b + c < 2 ** 512 for a, b, c in items)
    out = pr.lane(name, [words8(a) + words8(b) + words8(c) for a, b, c in items])
    for (a, b, c), o in zip(items, out):
        assert int_of(o) == (a * b + c) % L, (name, hex(a), hex(b), hex(c))
    return len(items)


def check_recode(pr, name):
    rng = random.Random(18)
    xs = [0, 1, L - 1, 2 ** 253 - 1, int("7" * 64, 16) % 2 ** 253, int("8" * 64, 16) % 2 ** 253]
    xs += [rng.getrandbits(253) for _ in range(1000)]
    out = pr.lane(name, [words8(x) for x in xs])
    if name == "recode16":
        for x, o in zip(xs, out):
            dg = [signed(w) for w in o]
            assert all(-8 <= t <= 7 for t in dg) and sum(t << (4 * i) for i, t in enumerate(dg)) == x, (name, hex(x))
        return len(xs)
    w = pr.base_w if name == "comb_base" else int(name[4:])
    rows, half = -(-254 // w), 1 << (w - 1)
    for x, o in zip(xs, out):
        assert int(o[0]) == rows
        dg = [signed(t) for t in o[1:1 + rows]]
        assert all(-half <= t < half for t in dg), (name, hex(x))
        assert sum(t << (w * i) for i, t in enumerate(dg)) == x, (name, hex(x))
        assert not o[1 + rows:].any()
    return len(xs)


# ---- points
def decode_ref(s, negate):
    """libsodium 1.0.18's ge25519_frombytes_negate_vartime on the integer s (negate = False: the
    point itself): y is the low 255 bits, not reduced and not checked against p; x is the root of
    (y^2 - 1) / (d y^2 + 1) whose parity is the sign bit (negate: the other one); x = 0 decodes
    with either sign bit.  None where there is no root."""
    y, sign = (s & (2 ** 255 - 1)) % p, s >> 255
    u, v = (y * y - 1) % p, (d * y * y + 1) % p
    x2 = u * E.inv(v) % p
    x = pow(x2, (p + 3) // 8, p)
    if (x * x - x2) % p:
        x = x * E.SQRTM1 % p
    if (x * x - x2) % p:
        return None
    if x and (x & 1) != (sign ^ int(negate)):
        x = p - x
    return (x, y)


@functools.lru_cache(None)
def blacklist():
    """libsodium's ge25519_has_small_order list as y values (the sign bit is masked before the
    comparison): 0, 1, the two order-8 y, p - 1, p, p + 1"""
    o8 = sorted({P[1] for P in E.order8_points() if E.mul(4, P) != E.IDENTITY})
    assert len(o8) == 2
    return [0, 1] + o8 + [p - 1, p, p + 1]


def small_order_ref(s):
    return (s & (2 ** 255 - 1)) in blacklist()


@functools.lru_cache(None)
def encodings():
    """The encodings for the decoders, as 256-bit integers"""
    rng = random.Random(23)
    out = [int.from_bytes(E.encode(P), "little") for P in E.order8_points()]
    out += [y | (s << 255) for y in blacklist() for s in (0, 1)]
    out += [(p + k) | (s << 255) for k in range(19) for s in (0, 1)]  # the 38 non-canonical y
    out += [y | (s << 255) for y in (0, 1, 2, p - 1, p - 2) for s in (0, 1)]  # with x = 0 and the sign bit set
    no_root = [y for y in range(2, 200) if decode_ref(y, False) is None][:16]
    assert len(no_root) == 16
    out += [y | (s << 255) for y in no_root for s in (0, 1)]
    out += [rng.getrandbits(256) for _ in range(2000)]
    return out


def p3_of(P, z=1):
    """affine P as X, Y, Z, T limbs (canonical splits) with Z = z"""
    x, y = P
    return canon_limbs(x * z % p) + canon_limbs(y * z % p) + canon_limbs(z % p) + canon_limbs(x * y * z % p)


def niels_of(P):
    x, y = P
    return canon_limbs((y + x) % p) + canon_limbs((y - x) % p) + canon_limbs(2 * d * x * y % p)


def affine_of(o):
    """a device point's 40 words -> affine (x, y), after the checks every result must pass: limbs
    in class C, Z != 0, T Z = X Y"""
    X, Y, Z, T = (val(o[10 * k:10 * k + 10]) % p for k in range(4))
    assert in_class(o[:10], C_MAX) and in_class(o[10:20], C_MAX) and in_class(o[20:30], C_MAX) and \
        in_class(o[30:40], C_MAX), list(o)
    assert Z != 0 and (T * Z - X * Y) % p == 0, list(o)
    zi = E.inv(Z)
    return (X * zi % p, Y * zi % p)


def check_frombytes(pr):
    enc = encodings()
    items = [(s, neg) for s in enc for neg in (0, 1)]
    out = pr.lane("ge_frombytes", [words8(s) + [neg] for s, neg in items])
    n_ok = 0
    for (s, neg), o in zip(items, out):
        want = decode_ref(s, bool(neg))
        assert int(o[0]) == int(want is not None), (hex(s), neg)
        X, Y, Z, T = (val(o[1 + 10 * k:11 + 10 * k]) % p for k in range(4))
        if want is None:
            assert (X, Y, Z, T) == (0, 1, 1, 0), hex(s)  # "a well-formed point": the identity
            continue
        n_ok += 1
        assert (X, Y, Z, T) == (want[0], want[1], 1, want[0] * want[1] % p), (hex(s), neg)
        assert all(in_class(o[1 + 10 * k:11 + 10 * k], C_MAX) for k in range(4))
    assert 100 < n_ok < len(items) - 100  # both outcomes
    return len(items)


def check_predicates(pr, name):
    xs = []
    for y in blacklist():
        for s in (0, 1):
            e = y | (s << 255)
            xs += [e] + [e ^ (1 << b) for b in range(256)]  # every one-bit neighbour
    xs += [(p + k) | (s << 255) for k in range(-2, 19) for s in (0, 1)] + encodings()[:200]
    out = pr.lane(name, [words8(x) for x in xs])
    for x, o in zip(xs, out):
        want = small_order_ref(x) if name == "has_small_order" else (x & (2 ** 255 - 1)) < p
        assert int(o[0]) == int(want), (name, hex(x))
    return len(xs)


@functools.lru_cache(None)
def random_points():
    """256 points of the prime-order subgroup with unrelated discrete logarithms"""
    rng = random.Random(25)
    out, step = [E.mul(rng.randrange(1, L), E.B)], E.mul(rng.randrange(1, L), E.B)
    while len(out) < 256:
        out.append(E.add(out[-1], step))
    return out


@functools.lru_cache(None)
def operand_points():
    """S of the issue: identity, B, -B, 2B, the order-2 point, both order-4 points, one order-8
    point, B + T8, six random points"""
    rng = random.Random(26)
    o8 = [P for P in E.order8_points() if E.mul(4, P) != E.IDENTITY][0]
    S = [E.IDENTITY, E.B, E.neg(E.B), E.add(E.B, E.B), (0, p - 1), (E.SQRTM1, 0), (p - E.SQRTM1, 0), o8,
         E.add(E.B, o8)]
    return S + rng.sample(random_points(), 6)


def check_group(pr, name):
    rng = random.Random(2600 + OP[name])
    S = operand_points()
    z = lambda: rng.randrange(1, p)  # noqa: E731
    if name in ("p2_dbl", "p3_dbl"):
        items = [(P, zz) for P in S for zz in (1, z(), p - 1)]
        out = pr.lane(name, [p3_of(P, zz) for P, zz in items])
        for (P, _), o in zip(items, out):
            assert affine_of(o) == E.add(P, P), (name, P)
        return len(items)
    if name == "comb_set_entry":
        items = [(P, e) for P in S for e in (1, 5, 2 ** 23, -1, -7, -2 ** 23)]
        rows = [niels_of(P) + [e & 0xffffffff] for P, e in items] + [canon_limbs(1) + canon_limbs(1) + [0] * 10 + [0]]
        out = pr.lane(name, rows)
        for (P, e), o in zip(items, out):
            assert affine_of(o) == (P if e > 0 else E.neg(P)), (name, P, e)
        assert affine_of(out[-1]) == E.IDENTITY  # the identity entry (1, 1, 0), e = 0
        return len(rows)
    if name == "ge_tobytes":
        items = [(P, zz) for P in S for zz in (1, 2, z(), z(), p - 1)]
        out = pr.lane(name, [p3_of(P, zz)[:30] for P, zz in items])
        for (P, _), o in zip(items, out):
            assert int_of(o) == int.from_bytes(E.encode(P), "little"), (name, P)
        return len(items)
    pairs = [(P, Q) for P in S for Q in S]  # every ordered pair: P + P, P + (-P), P + O, torsion
    if name in ("ge_madd", "ge_msub"):
        rows = [p3_of(P, z() if i % 2 else 1) + niels_of(Q) for i, (P, Q) in enumerate(pairs)]
        want = [E.add(P, Q if name == "ge_madd" else E.neg(Q)) for P, Q in pairs]
    elif name == "ge_add_signed":
        pairs = [(P, Q, neg) for P, Q in pairs for neg in (0, 1)]
        rows = [p3_of(P, z()) + p3_of(Q, z() if i % 2 else 1) + [neg] for i, (P, Q, neg) in enumerate(pairs)]
        want = [E.add(P, E.neg(Q) if neg else Q) for P, Q, neg in pairs]
    else:
        rows = [p3_of(P, z() if i % 2 else 1) + p3_of(Q, z() if i % 3 else 1) for i, (P, Q) in enumerate(pairs)]
        want = [E.add(P, Q if name == "ge_add" else E.neg(Q)) for P, Q in pairs]
    out = pr.lane(name, rows)
    for pq, w, o in zip(pairs, want, out):
        assert affine_of(o) == w, (name, pq)
    return len(rows)


def check_walk(pr, steps=200, every=20):
    """One random walk of add / dbl / madd, each step fed the previous step's output limbs as they
    are; compared with the Python walk every `every` steps."""
    rng = random.Random(33)
    S = operand_points()
    cur, ref = p3_of(E.B, rng.randrange(1, p)), E.B
    for step in range(1, steps + 1):
        kind = rng.choice(["ge_add", "p3_dbl", "ge_madd"])
        Q = rng.choice(S) if rng.random() < 0.5 else rng.choice(random_points())
        if kind == "ge_add":
            row, ref = cur + p3_of(Q, rng.randrange(1, p)), E.add(ref, Q)
        elif kind == "ge_madd":
            row, ref = cur + niels_of(Q), E.add(ref, Q)
        else:
            row, ref = cur, E.add(ref, ref)
        o = pr.lane(kind, [row])[0]
        cur = [int(v) for v in o]
        if step % every == 0:
            assert affine_of(o) == ref, step
    return steps


# ---- hash
def hash_lengths():
    edge = sorted({128 * b - 81 + dl for b in range(34) for dl in (-2, -1, 0, 1) if 0 <= 128 * b - 81 + dl <= 4200})
    return edge, sorted(set(range(301)) | set(edge))


def _hash_requests(n, rng):
    """S, R, A of n requests from the canonicity and blacklist edges as well as random values: the
    flag has both outcomes"""
    bl = blacklist()
    sig, pk, ok = [], [], []
    for i in range(n):
        kind = i % 10
        S = [rng.randrange(L), L - 1, 0, rng.randrange(L), rng.randrange(L), rng.randrange(L), L, L + 1, 2 ** 256 - 1,
             rng.randrange(L)][kind]
        R, A = rng.getrandbits(256), rng.getrandbits(255) % p | (rng.getrandbits(1) << 255)
        if kind == 3:
            R = bl[i % 7] | (rng.getrandbits(1) << 255)
        if kind == 4:
            A = (p + rng.randrange(19)) | (rng.getrandbits(1) << 255)
        if kind == 5:
            A = bl[i % 7] | (rng.getrandbits(1) << 255)
        if kind == 9:
            R = (bl[i % 7] ^ (1 << rng.randrange(255))) | (rng.getrandbits(1) << 255)  # a neighbour: not listed
        sig.append(R.to_bytes(32, "little") + S.to_bytes(32, "little"))
        pk.append(A.to_bytes(32, "little"))
        ok.append(S < L and not small_order_ref(R) and (A & (2 ** 255 - 1)) < p and not small_order_ref(A))
    return sig, pk, ok


def check_hash(pr, form):
    """h = int(sha512(R || A || M), little) mod L and flag = the four prechecks, message i at
    alignment i mod 16 (the lanes form: every edge length at all 16 alignments), the bytes around
    every message inside the 16-byte chunks the loader reads once 0x00 and once 0xFF."""
    rng = random.Random(40 + form)
    edge, lens = hash_lengths()
    if form == 2:
        cases = [(n, a) for n in edge for a in range(16)] + [(n, i % 16) for i, n in enumerate(range(301))]
    else:
        cases = [(n, i % 16) for i, n in enumerate(lens)]
    sig, pk, ok = _hash_requests(len(cases), rng)
    assert any(ok) and not all(ok)
    msgs = [bytes(rng.getrandbits(8) for _ in range(n)) if n < 400 else rng.getrandbits(8 * n).to_bytes(n, "little")
            for n, _ in cases]
    want = [int.from_bytes(hashlib.sha512(s[:32] + k + m).digest(), "little") % L for s, k, m in zip(sig, pk, msgs)]
    got = []
    for fill in (0x00, 0xff):
        buf, start = bytearray(), []
        for (n, a), m in zip(cases, msgs):
            buf += bytes([fill]) * (16 + a)  # a chunk of fill, then the message's own chunk up to it
            start.append(len(buf))
            buf += m
            buf += bytes([fill]) * (-len(buf) % 16)
        buf += bytes([fill]) * 16
        assert all(s % 16 == a for s, (_, a) in zip(start, cases))
        h, flag = pr.hash(form, sig, pk, buf, start, [n for n, _ in cases])
        for i, (n, a) in enumerate(cases):
            assert h[i] == want[i], (form, fill, n, a)
            assert flag[i] == ok[i], (form, fill, n, a)
        got.append(h)
    assert got[0] == got[1]
    return len(cases)


# ---- the lane forms (device only; the CPU reference is the model of test_fe_lanes_model.py)
JUNK = 0xffffffff


def check_model_exact():
    """The reference of the lane forms against integers, on the very inputs the device gets: the
    model's carry(columns(...)) is the square / the product mod p and stays inside its bounds."""
    ins = lane_inputs()
    for t, f in enumerate(ins):
        g = ins[(7 * t + 3) % len(ins)]
        r = M.carry(M.columns(f, f, M.SQ))
        assert M.value(r) == M.value(f) ** 2 % p and M.in_bounds(r), f
        r = M.carry(M.columns(f, g, M.MU))
        assert M.value(r) == M.value(f) * M.value(g) % p and M.in_bounds(r), (f, g)
    return 2 * len(ins)


def lane_products(f, g, tab):
    """the 64 lanes' sums of products before lane_cols_carry (the model's columns(), by lane)"""
    out = [0] * 64
    for lane in range(64):
        for i, j, ma, mb in tab[lane]:
            a, b = f[i] * ma, g[j] * mb
            assert a < 2 ** 32 and b < 2 ** 32
            out[lane] += a * b
        assert out[lane] < 2 ** 64
    return out


def _spread(limbs, junk):
    """limb k in lane k; lanes 10..63 zero or all ones"""
    return list(limbs) + [JUNK if junk else 0] * 54


def lane_inputs():
    """the model's extreme() and its class-C list"""
    rng = random.Random(7)
    out = [M.extreme(rng) for _ in range(400)]
    r2 = random.Random(11)
    out += [canon_limbs(x) for x in [0, 1, 2, 19, p - 1, p - 2, 2 ** 255 - 20] + [r2.randrange(p) for _ in range(200)]]
    top = [2 ** 26 - 1, M.BOUND_1 - 1] + [(M.BOUND_EVEN if k % 2 == 0 else M.BOUND_ODD) - 1 for k in range(2, 10)]
    return out + [top]


def check_dist(pr, name):
    """dist_sq / dist_mul / dist_sqn / lane_cols_carry: lanes 0..9 equal the model's
    carry(columns(...)) limb for limb and stay inside its bounds; half the cases with 0xffffffff in
    the input lanes 10..63 (lane_cols_carry: in the lanes of columns 10..15)."""
    ins = lane_inputs()
    rng = random.Random(50 + WOP[name])
    if name == "dist_sq":
        rows = [_spread(f, t & 1) for t, f in enumerate(ins)]
        want = [M.carry(M.columns(f, f, M.SQ)) for f in ins]
        out = pr.wave(name, rows)
    elif name == "dist_mul":
        gs = [ins[rng.randrange(len(ins))] for _ in ins]
        rows = [_spread(f, t & 1) + _spread(g, (t >> 1) & 1) for t, (f, g) in enumerate(zip(ins, gs))]
        want = [M.carry(M.columns(f, g, M.MU)) for f, g in zip(ins, gs)]
        out = pr.wave(name, rows)
    elif name == "dist_sqn":
        n, rows = 0, [_spread(f, t & 1) for t, f in enumerate(ins)]
        for nsq in (1, 2, 5, 30):
            w = []
            for f in ins:
                r = f
                for _ in range(nsq):
                    r = M.carry(M.columns(r, r, M.SQ))
                w.append(r)
            o = pr.wave(name, rows, aux=nsq)
            for f, ww, oo in zip(ins, w, o):
                assert list(map(int, oo[:10])) == ww and M.in_bounds(ww), (name, nsq, f)
            n += len(rows)
        return n
    else:
        assert name == "cols_carry"
        rows, want = [], []
        for t, f in enumerate(ins):
            g = ins[rng.randrange(len(ins))]
            tab = M.SQ if t % 3 else M.MU
            pl = lane_products(f, f if t % 3 else g, tab)
            if t & 1:
                for lane in range(64):
                    if lane % 16 >= 10:
                        pl[lane] = 2 ** 64 - 1
            rows.append([v & 0xffffffff for v in pl] + [v >> 32 for v in pl])
            want.append(M.carry(M.columns(f, f if t % 3 else g, tab)))
        out = pr.wave(name, rows)
    for f, w, o in zip(ins, want, out):
        assert list(map(int, o[:10])) == w, (name, f, list(o[:10]), w)
        assert M.in_bounds(w)
    return len(rows)


def check_dist_chains(pr, trials=40, steps=60):
    """The model's own test, run on the device: chains of mixed squares and products from limbs at
    the output bounds, every step's lanes 0..9 equal to the model's and inside its bounds."""
    rng = random.Random(7)
    fs, gs = [], []
    for _ in range(trials):
        fs.append(M.extreme(rng))
        gs.append(M.extreme(rng))
    n = 0
    for step in range(steps):
        sq = [rng.random() < 0.8 for _ in range(trials)]
        isq, imu = [t for t in range(trials) if sq[t]], [t for t in range(trials) if not sq[t]]
        res = [None] * trials
        if isq:
            o = pr.wave("dist_sq", [_spread(fs[t], (t + step) & 1) for t in isq])
            for t, oo in zip(isq, o):
                res[t] = list(map(int, oo[:10]))
                assert res[t] == M.carry(M.columns(fs[t], fs[t], M.SQ)), (step, t)
        if imu:
            o = pr.wave("dist_mul", [_spread(fs[t], (t + step) & 1) + _spread(gs[t], t & 1) for t in imu])
            for t, oo in zip(imu, o):
                res[t] = list(map(int, oo[:10]))
                assert res[t] == M.carry(M.columns(fs[t], gs[t], M.MU)), (step, t)
        for t in range(trials):
            assert M.in_bounds(res[t])
            fs[t] = res[t] if rng.random() < 0.7 else M.extreme(rng)
        n += trials
    return n


def check_dist_round(pr):
    """dist_from_lane0 -> dist_to_fe: lane 0's class-C element comes back, carried, in every lane;
    the other lanes' inputs are ignored."""
    rng = random.Random(54)
    fs = edge_patterns(C_MAX) + random_patterns(C_MAX, rng, 64)
    rows = []
    for t, f in enumerate(fs):
        other = [JUNK] * 10 if t & 1 else [0] * 10
        rows.append(list(f) + other * 63)
    out = pr.wave("dist_round", rows)
    for f, o in zip(fs, out):
        assert list(map(int, o[:10])) == list(f) and not o[10:64].any(), f
        w = carry_ref(f)
        for lane in range(64):
            assert list(map(int, o[64 + 10 * lane:74 + 10 * lane])) == w, (f, lane)
    return len(rows)


def carry_ref(f):
    """fe_carry on integers"""
    h = list(f)
    for k in range(9):
        h[k + 1] += h[k] >> WID[k]
        h[k] &= (1 << WID[k]) - 1
    c = h[9] >> 25
    h[9] &= (1 << 25) - 1
    h[0] += 19 * c
    h[1] += h[0] >> 26
    h[0] &= (1 << 26) - 1
    return h


def check_r_decode(pr):
    """R's decode on the lanes: the flag and the bytes of x equal the one-lane ge_frombytes
    (negate = false) on the same device and Python; x is unspecified where the flag is false."""
    enc = encodings()
    out = pr.wave("r_decode", [words8(s) for s in enc])
    one = pr.lane("ge_frombytes", [words8(s) + [0] for s in enc])
    n_ok = 0
    for s, o, l in zip(enc, out, one):
        want = decode_ref(s, False)
        assert int(o[0]) == int(l[0]) == int(want is not None), hex(s)
        if want is not None:
            n_ok += 1
            assert int_of(o[1:9]) == val(l[1:11]) % p == want[0], hex(s)
    assert 100 < n_ok < len(enc) - 100
    return len(enc)


def check_tree_sum(pr, width):
    rng = random.Random(60 + width)
    S = operand_points()
    ident = E.IDENTITY
    rp = lambda: rng.choice(random_points())  # noqa: E731
    tors = E.order8_points()
    cases = [[ident] * width]
    for pos in range(width):  # one point at each lane position: the result is that point
        P = S[1 + pos % (len(S) - 1)]
        cases.append([P if k == pos else ident for k in range(width)])
    P = rp()
    cases.append([P] * width)                                         # every level doubles: [width]P
    cases.append([S[7]] * width)                                      # ... of an order-8 point
    cases.append([P if k % 2 == 0 else E.neg(P) for k in range(width)])  # the identity, Z != 0
    cases.append([P if k % 4 < 2 else E.neg(P) for k in range(width)])
    for _ in range(4):
        cases.append([rng.choice(tors) if rng.random() < 0.5 else rp() for _ in range(width)])  # torsion mixed in
    for _ in range(4):
        cases.append([rp() for _ in range(width)])
    want = []
    for c in cases:
        acc = ident
        for Q in c:
            acc = E.add(acc, Q)
        want.append(acc)
    assert want[width + 1] == E.mul(width, P) and want[width + 3] == ident
    n = 0
    for junk in (False, True):  # lanes >= width: the identity, then non-identity points that must not matter
        rows = []
        for c in cases:
            row = []
            for k in range(64):
                Q = c[k] if k < width else (rp() if junk and k % 8 == 0 else S[3] if junk else ident)
                row += p3_of(Q, rng.randrange(1, p) if k % 2 else 1)
            rows.append(row)
        out = pr.wave("tree_sum", rows, aux=width)
        for i, (w, o) in enumerate(zip(want, out)):
            assert affine_of(o) == w, (width, junk, i)
        n += len(rows)
    return n


# ---- signature slots (csrc/sig_slot.h: the body of edv_b58_sig_kernel)
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def b58encode(raw):
    """the base58 text of raw: a '1' per leading zero byte, then the digits of the rest's value"""
    nz = len(raw) - len(raw.lstrip(b"\0"))
    v, digits = int.from_bytes(raw, "big"), ""
    while v:
        v, r = divmod(v, 58)
        digits = B58[r] + digits
    return "1" * nz + digits


def sig_slot_values():
    """64-byte signatures with nz = 0..64 leading zero bytes: the smallest and the largest value of
    the other L = 64 - nz bytes, 01 ff.., ff 00.. and 20 random ones with a non-zero top byte"""
    rng = random.Random(58)
    out = []
    for nz in range(65):
        n = 64 - nz
        if n == 0:
            out.append(bytes(64))
            continue
        tails = [b"\x01" + bytes(n - 1), b"\xff" * n, b"\x01" + b"\xff" * (n - 1), b"\xff" + bytes(n - 1)]
        tails += [bytes([rng.randrange(1, 256)]) + bytes(rng.getrandbits(8) for _ in range(n - 1)) for _ in range(20)]
        out += [bytes(nz) + t for t in tails]
    return out


def sig_slot_text_lengths(values):
    return [len(b58encode(v)) for v in values]


def check_sig_slot(pr):
    """A text slot decodes to the 64 bytes it encodes, whatever follows the text up to byte 95; a
    raw slot (byte 95 = 0) passes its first 64 bytes through, whatever bytes 64..94 hold."""
    values = sig_slot_values()
    rng = random.Random(59)
    rows, want = [], []
    for v in values:
        text = b58encode(v).encode()
        assert 64 <= len(text) <= 88
        for fill in (b"\0", b"z"):
            rows.append(text + fill * (95 - len(text)) + bytes([len(text)]))
            want.append(v)
    for v in values[::7] + [b"\xff" * 64, bytes(64)]:
        for fill in (bytes(31), b"z" * 31, bytes(rng.getrandbits(8) for _ in range(31))):
            rows.append(v + fill + b"\0")
            want.append(v)
    a = np.frombuffer(b"".join(rows), "<u4").reshape(len(rows), 24)
    got = pr.lane("sig_slot", a).astype("<u4")
    for i, v in enumerate(want):
        assert got[i].tobytes() == v, (i, rows[i][95], rows[i][:rows[i][95]], v.hex(), got[i].tobytes().hex())
    return len(rows)
