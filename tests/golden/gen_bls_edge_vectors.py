"""Generate tests/golden/bls_edge_vectors.json from the CPU BLS oracle
(oracle/bls_bn254_oracle.py): the edges of the BLS check -- scalars at the ends
of the ladder, messages on SHA-256 padding boundaries and on H(m)'s
try-and-increment edges, repeated and cancelling verkeys and signatures,
encodings with a coordinate >= p, a second generator -- for
tests/test_bls_edges.py (the CPU build of the device code) and
tests/test_gpu_bls_edges.py (the kernels).

Every expectation is the oracle's answer over the wire bytes; next to it the
generator asserts the verdict the construction implies, so a wrong oracle call
cannot define the truth.  Every distinct 128-byte value is stored once
("points") and named by index.  Fixed seed, deterministic output.

usage: python tests/golden/gen_bls_edge_vectors.py"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls_bn254_oracle as o  # noqa: E402

R, P = o.R, o.P
OUT_OF_CONTRACT = "outside the header's sk < r contract; pins the infinity and P + (-P) branches of the ladder"
REDO_MSG = b"wave-form redo 11075"  # tests/test_gpu_bls.py: the first point is past candidate 16

EDGE_SKS = [("1", 1), ("2", 2), ("3", 3), ("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2),
            ("(r+1)/2", (R + 1) // 2), ("2^31", 1 << 31), ("2^32", 1 << 32), ("2^63", 1 << 63), ("2^64", 1 << 64),
            ("2^128", 1 << 128), ("2^253", 1 << 253), ("2^253-1", (1 << 253) - 1),
            ("0x55..55 mod r", int("55" * 32, 16) % R), ("0xaa..aa mod r", int("aa" * 32, 16) % R)]
N_RANDOM, N_EXTRA = 4, 5  # 4 random keys; 5 more only to fill the 25-verkey multi-signature
MSG_LENGTHS = [0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129, 183, 184, 1000]
CANDIDATES = [1, 2, 3, 7, 8, 15, 16]

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


def first_candidate(msg):
    """(q, c): floor(SHA-256(m) / p) and the try-and-increment candidate that is H(m)'s x."""
    h = int.from_bytes(hashlib.sha256(msg).digest(), "big")
    c = 0
    while not o._is_square((((h + c) % P) ** 3 + o.B1) % P):
        c += 1
    return h // P, c


def f2_sqrt(c):
    """A square root of c in Fp2 = Fp[i]/(i^2 + 1) (p = 3 mod 4), or None: (s + t i)^2 = c from
    s^2 = (c.a +- |c|) / 2, t = c.b / 2s.  Only builds an input; the result is checked by squaring."""
    n = (c.a * c.a + c.b * c.b) % P
    if not o._is_square(n):
        return None
    n = o._sqrt_p(n)
    for s2 in ((c.a + n) * pow(2, P - 2, P) % P, (c.a - n) * pow(2, P - 2, P) % P):
        if o._is_square(s2):
            s = o._sqrt_p(s2)
            y = o.F2(s, c.b * pow(2 * s, P - 2, P))
            if y * y == c:
                return y
    return None


def main():
    rng = random.Random(20261020)
    points, index = [], {}

    def pt(b):
        b = bytes(b)
        assert len(b) == 128
        if b not in index:
            index[b] = len(points)
            points.append(b.hex())
        return index[b]

    gen = o.generator()
    gen_b = o.g2_to_bytes(gen)
    gen7 = o.g2_mul(gen, 7)
    gen_off = bytearray(gen_b)
    gen_off[70] ^= 1
    assert o.g2_from_bytes(bytes(gen_off)) is None and o.g2_from_bytes(b"\0" * 128) is None
    gens_b = [gen_b, o.g2_to_bytes(gen7), b"\0" * 128, bytes(gen_off)]
    generators = [{"name": n, "g": pt(b)} for n, b in zip(("reference", "[7]g", "zero", "off_curve"), gens_b)]

    # ---------------------------------------------------------------- keys
    sks = list(EDGE_SKS) + [("random %d" % i, rng.randrange(1, R)) for i in range(N_RANDOM)]
    n_edge_keys = len(sks)
    sks += [("extra %d (25-verkey multi-signature only)" % i, rng.randrange(1, R)) for i in range(N_EXTRA)]
    assert len(sks) == 25 and all(0 < sk < R for _, sk in sks)
    keys = [{"name": n, "sk": "%064x" % sk, "gen": 0, "vk": pt(o.g2_to_bytes(o.keygen(sk, gen))), "in_contract": True}
            for n, sk in sks]
    assert points[keys[0]["vk"]] == gen_b.hex()
    assert points[keys[3]["vk"]] == o.g2_to_bytes(o.g2_neg(gen)).hex()
    G7 = [len(keys), len(keys) + 1]  # keys over the second generator
    for i in range(2):
        sk = rng.randrange(1, R)
        sks.append(("over [7]g %d" % i, sk))
        keys.append({"name": sks[-1][0], "sk": "%064x" % sk, "gen": 1, "vk": pt(o.g2_to_bytes(o.keygen(sk, gen7))),
                     "in_contract": True})
    OOC = []
    for n, sk in (("0", 0), ("r", R), ("r+1", R + 1)):
        OOC.append(len(keys))
        sks.append((n, sk))
        want = o.g2_mul(gen, sk % R)
        assert o.keygen(sk, gen) == want
        keys.append({"name": n, "sk": "%064x" % sk, "gen": 0, "vk": pt(o.g2_to_bytes(want)), "in_contract": False,
                     "label": OUT_OF_CONTRACT})
    assert points[keys[OOC[0]]["vk"]] == points[keys[OOC[1]]["vk"]] == "00" * 128
    assert keys[OOC[2]]["vk"] == keys[0]["vk"]
    # A coordinate equal to p exactly, where the reduced value is a point: no G1 or subgroup
    # point has a zero coordinate (2 is no square mod p, no point has order 2), so a twist
    # point (0 + b i, y) outside the subgroup, as a generator, its x.a written as p.  The
    # output bytes tell infinity (zeros) from the point, which no verdict would.
    b = 1
    while True:
        x = o.F2(0, b)
        y = f2_sqrt(x * x * x + o.B2)
        if y is not None:
            break
        b += 1
    on_twist = o.g2_to_bytes((x, y))
    assert o.g2_from_bytes(on_twist) == (x, y) and on_twist[:32] == b"\0" * 32
    xa_p = P.to_bytes(32, "big") + on_twist[32:]
    assert o.g2_from_bytes(xa_p) is None
    for name, gb in (("x.a = 0 (on the twist)", on_twist), ("x.a = p exactly", xa_p)):
        generators.append({"name": name, "g": pt(gb)})
        gens_b.append(gb)
        for sk in (1, 2):
            sks.append(("%d over the generator with %s" % (sk, name), sk))
            want = o.keygen(sk, o.g2_from_bytes(gb))
            assert (want is None) == (gb is xa_p) and (sk != 1 or gb is xa_p or want == (x, y))
            keys.append({"name": sks[-1][0], "sk": "%064x" % sk, "gen": len(gens_b) - 1, "vk": pt(o.g2_to_bytes(want)),
                         "in_contract": True})

    # ---------------------------------------------------------------- messages
    msgs = []  # (name, bytes)
    for n in MSG_LENGTHS:
        msgs.append(("length %d" % n, bytes(rng.getrandbits(8) for _ in range(n))))
    want_q, want_c, t = set(range(7)), set(CANDIDATES), 0
    found_q, found_c = {}, {}
    while want_q or want_c:
        m = b"bls edge search %d" % t
        t += 1
        q, c = first_candidate(m)
        if q in want_q:
            want_q.discard(q)
            found_q[q] = m
        elif c in want_c:
            want_c.discard(c)
            found_c[c] = m
    searched = t
    msgs += [("digest in [%dp, %dp)" % (q, q + 1), found_q[q]) for q in range(7)]
    msgs += [("first point at candidate %d" % c, found_c[c]) for c in CANDIDATES]
    msgs.append(("first point past candidate 16 (REDO_MSG)", REDO_MSG))
    messages = []
    for n, m in msgs:
        q, c = first_candidate(m)
        h = o.hash_to_g1(m)
        assert h[0] == (int.from_bytes(hashlib.sha256(m).digest(), "big") + c) % P
        messages.append({"name": n, "hex": m.hex(), "q": q, "candidate": c, "h": pt(o.g1_to_bytes(h))})
    assert [x["q"] for x in messages[18:25]] == list(range(7))
    assert [x["candidate"] for x in messages[25:32]] == CANDIDATES and messages[32]["candidate"] > 16
    M_C15, M_C16, M_REDO = 30, 31, 32

    # ---------------------------------------------------------------- signatures
    sig_pts, signatures = {}, []

    def sig_of(k, m):
        if (k, m) not in sig_pts:
            s = o.sign(msgs[m][1], sks[k][1])
            assert s == o.g1_mul(o.hash_to_g1(msgs[m][1]), sks[k][1] % R)
            sig_pts[(k, m)] = s
            signatures.append({"key": k, "msg": m, "sig": pt(o.g1_to_bytes(s))})
        return sig_pts[(k, m)]

    def sigb(k, m):
        return o.g1_to_bytes(sig_of(k, m))

    def vkb(k):
        return bytes.fromhex(points[keys[k]["vk"]])

    # every edge key and every message in a valid check: key i on message i, the remaining
    # messages on keys in turn
    pairs = [(i, i) for i in range(n_edge_keys)] + [(m % n_edge_keys, m) for m in range(n_edge_keys, len(msgs))]
    for k in OOC:  # sign only
        for m in (2, 19):
            s = sig_of(k, m)
            assert (s is None) == (sks[k][1] % R == 0)
    assert sig_pts[(OOC[2], 2)] == o.hash_to_g1(msgs[2][1])

    # ---------------------------------------------------------------- verdict cases
    cases = []

    def add(name, cls, sig, m, vk_list, implied, g=0):
        assert cls in CASE_CLASSES, cls
        expect = o.verify_multi_bytes(sig, msgs[m][1], vk_list, gens_b[g])
        assert expect is implied, (name, expect, implied)
        cases.append({"name": name, "class": cls, "sig": pt(sig), "msg": m, "vks": [pt(v) for v in vk_list], "gen": g,
                      "expect": bool(expect)})

    for k, m in pairs:
        cls = {0: "vk_generator", 3: "vk_neg_generator"}.get(k, "valid")
        add("valid key '%s' on '%s'" % (sks[k][0], msgs[m][0]), cls, sigb(k, m), m, [vkb(k)], True)
    for k in range(n_edge_keys):
        m2 = (k + 1) % len(msgs)
        add("key '%s': signature of message %d on message %d" % (sks[k][0], k, m2), "wrong_message", sigb(k, k), m2,
            [vkb(k)], False)
    for k in range(6):
        add("key %d's signature against key %d" % (k, k + 7), "wrong_key", sigb(k, k), k, [vkb(k + 7)], False)
    s, k, m = sig_of(16, 16), 16, 16
    add("[vk, vk] with 2 s", "dup_vk_sig_doubled", o.g1_to_bytes(o.g1_add(s, s)), m, [vkb(k), vkb(k)], True)
    add("[vk, vk] with s", "dup_vk_sig_single", o.g1_to_bytes(s), m, [vkb(k), vkb(k)], False)
    neg_vk = o.g2_to_bytes(o.g2_neg(o.g2_from_bytes(vkb(k))))
    add("[vk, -vk, vk2] with key 2's signature", "cancel_vk_plus_third", sigb(17, m), m, [vkb(k), neg_vk, vkb(17)], True)
    add("[vk, -vk]: the sum is infinity", "cancel_vk_sum_infinity", o.g1_to_bytes(s), m, [vkb(k), neg_vk], False)
    add("[generator, -generator, vk]", "cancel_vk_plus_third", sigb(5, 5), 5, [vkb(0), vkb(3), vkb(5)], True)
    add("a one-verkey list", "single_vk_list", sigb(4, 7), 7, [vkb(4)], True)
    add("a one-verkey list, wrong message", "single_vk_list", sigb(4, 7), 8, [vkb(4)], False)
    all25 = list(range(25))
    for m in (9, M_C16):
        agg = o.aggregate([sig_of(k, m) for k in all25])
        add("25 verkeys on message %d" % m, "multi25", o.g1_to_bytes(agg), m, [vkb(k) for k in all25], True)
        agg = o.aggregate([sig_of(k, m) for k in all25 if k != 11])
        add("25 verkeys, signer 11 missing, message %d" % m, "multi25_missing_signer", o.g1_to_bytes(agg), m,
            [vkb(k) for k in all25], False)
    add("signature -s", "neg_sig", o.g1_to_bytes(o.g1_neg(sig_of(18, 18))), 18, [vkb(18)], False)
    # G1 encodings
    sb = sigb(19, 19)
    x, y = sig_of(19, 19)
    add("G1 x + p", "sig_x_plus_p", b"\x04" + (x + P).to_bytes(32, "big") + sb[33:], 19, [vkb(19)], False)
    add("G1 y + p", "sig_y_plus_p", sb[:33] + (y + P).to_bytes(32, "big") + sb[65:], 19, [vkb(19)], False)
    add("G1 x = p exactly", "sig_x_equals_p", b"\x04" + P.to_bytes(32, "big") + sb[33:], 19, [vkb(19)], False)
    add("G1 x-only, x + p", "sig_x_plus_p", b"\x02" + (x + P).to_bytes(32, "big") + b"\0" * 95, 19, [vkb(19)], False)
    xn = x
    while o._is_square((xn ** 3 + o.B1) % P):
        xn += 1
    add("G1 first byte 2 over a non-residue x", "sig_xonly_nonresidue", b"\x02" + xn.to_bytes(32, "big") + sb[33:], 19,
        [vkb(19)], False)
    add("G1 0x04 | x | y with nonzero trailing bytes", "sig_trailing_bytes", sb[:65] + bytes(range(1, 64)), 19,
        [vkb(19)], True)
    # G2 encodings
    vb = vkb(19)
    for j, cls in enumerate(("vk_xa_plus_p", "vk_xb_plus_p", "vk_ya_plus_p", "vk_yb_plus_p")):
        c = int.from_bytes(vb[32 * j:32 * j + 32], "big") + P
        add("G2 coordinate %d + p" % j, cls, sb, 19, [vb[:32 * j] + c.to_bytes(32, "big") + vb[32 * j + 32:]], False)
        add("G2 coordinate %d + p beside the verkey itself" % j, cls, sb, 19,
            [vb[:32 * j] + c.to_bytes(32, "big") + vb[32 * j + 32:], vb], True)
    add("verkey with a / b swapped", "vk_ab_swapped", sb, 19, [vb[32:64] + vb[:32] + vb[96:] + vb[64:96]], False)
    # generators
    for k in G7:
        add("key %d over [7]g" % k, "second_generator", sigb(k, 3), 3, [vkb(k)], True, g=1)
    add("both keys over [7]g", "second_generator", o.g1_to_bytes(o.aggregate([sig_of(k, 4) for k in G7])), 4,
        [vkb(k) for k in G7], True, g=1)
    add("a key over g checked over [7]g", "second_generator_key_on_first", sigb(1, 1), 1, [vkb(1)], False, g=1)
    add("a key over [7]g checked over g", "second_generator_key_on_first", sigb(G7[0], 3), 3, [vkb(G7[0])], False)
    add("generator all zero", "generator_zero", sigb(1, 1), 1, [vkb(1)], False, g=2)
    add("generator off the curve", "generator_off_curve", sigb(1, 1), 1, [vkb(1)], False, g=3)

    # ---------------------------------------------------------------- aggregates
    aggregates = []

    def agg(name, cls, sig_list, implied):
        assert cls in AGG_CLASSES, cls
        out = o.g1_to_bytes(o.aggregate([o.g1_from_bytes(b) for b in sig_list]))
        assert out == o.g1_to_bytes(implied), name
        aggregates.append({"name": name, "class": cls, "sigs": [pt(b) for b in sig_list], "out": pt(out)})

    s, t2 = sig_of(16, 16), sig_of(17, 16)
    sB, nB, tB = o.g1_to_bytes(s), o.g1_to_bytes(o.g1_neg(s)), o.g1_to_bytes(t2)
    zero = b"\0" * 128
    off = b"\x04" + (7).to_bytes(32, "big") + b"\0" * 95
    assert o.g1_from_bytes(zero) is None and o.g1_from_bytes(off) is None
    agg("[s]", "single", [sB], s)
    agg("[s, s]", "doubled", [sB, sB], o.g1_mul(s, 2))
    agg("[s, s, s, s]", "doubled", [sB] * 4, o.g1_mul(s, 4))
    agg("[s, -s]", "cancel_to_zero", [sB, nB], None)
    agg("[s, -s, t]", "cancel_plus_third", [sB, nB, tB], t2)
    agg("[infinity, s]", "infinity_first", [zero, sB], s)
    agg("[s, infinity]", "infinity_last", [sB, zero], s)
    agg("[off-curve, s]", "off_curve_first", [off, sB], s)
    agg("[]", "empty", [], None)
    agg("25 terms", "n25", [sigb(k, 9) for k in all25], o.g1_mul(o.hash_to_g1(msgs[9][1]), sum(sk for _, sk in sks[:25])))
    xonly = bytes([2 + (s[1] & 1)]) + sB[1:33] + b"\0" * 95
    agg("[x-only s, t]", "x_only", [xonly, tB], o.g1_add((s[0], o._sqrt_p((s[0] ** 3 + o.B1) % P)), t2))

    # ---------------------------------------------------------------- conditions
    n_acc = sum(c["expect"] for c in cases)
    assert n_acc >= 40 and len(cases) - n_acc >= 40, (n_acc, len(cases))
    assert {c["class"] for c in cases} == set(CASE_CLASSES)
    assert {a["class"] for a in aggregates} == set(AGG_CLASSES)
    for k in range(n_edge_keys):
        assert any(c["expect"] and c["vks"] == [keys[k]["vk"]] for c in cases), k
    for m in range(len(msgs)):
        assert any(c["expect"] and c["msg"] == m for c in cases), m
    out = {
        "note": "generated by tests/golden/gen_bls_edge_vectors.py from oracle/bls_bn254_oracle.py; every 'expect', "
                "'out', 'vk', 'sig' and 'h' is the oracle's; 128-byte values are indices into 'points'",
        "points": points,
        "generators": generators,
        "keys": keys,
        "messages": messages,
        "signatures": signatures,
        "cases": cases,
        "aggregates": aggregates,
        "case_classes": CASE_CLASSES,
        "aggregate_classes": AGG_CLASSES,
        "special_messages": {"candidate_15": M_C15, "candidate_16": M_C16, "redo": M_REDO},
    }
    path = os.path.join(HERE, "bls_edge_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %d points, %d keys, %d messages (%d searched), %d signatures" %
          (os.path.basename(path), len(points), len(keys), len(messages), searched, len(signatures)))
    print("cases: %d accept, %d reject; aggregates: %d" % (n_acc, len(cases) - n_acc, len(aggregates)))
    for cls in CASE_CLASSES:
        print("  %-32s %d" % (cls, sum(c["class"] == cls for c in cases)))
    for cls in AGG_CLASSES:
        print("  aggregate %-22s %d" % (cls, sum(a["class"] == cls for a in aggregates)))


if __name__ == "__main__":
    main()
