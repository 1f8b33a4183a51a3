"""The BLS device code's edges on the CPU (bn254.h / bls_wave.h compiled into
libedv_hostcheck.so), bit for bit against the oracle's edge fixture
(tests/golden/bls_edge_vectors.json) and, for the Fp primitives, against Python integers:
the CPU twins of tests/test_gpu_bls_edges.py and tests/test_gpu_bls_fp.py.  A failure there
alone is the device's; one here too is the arithmetic's."""
import ctypes

import pytest

import bls_edge_common as ec
from bls_edge_common import o

U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def fx():
    return ec.fixture()


@pytest.fixture(scope="module")
def hc(hostcheck):
    hostcheck.edv_host_bls_verify.restype = ctypes.c_int
    hostcheck.edv_host_bls_verify_program.restype = ctypes.c_int
    hostcheck.edv_host_bn_fp.restype = ctypes.c_int
    hostcheck.edv_host_blsp_exec.restype = ctypes.c_int
    return hostcheck


def test_fixture_conditions(fx):
    """At least 40 accepting and 40 rejecting cases, every class by name, every edge key and
    message in an accepting check."""
    fx.check_conditions()


def test_fixture_expectations_are_the_oracles(fx):
    """A few cases of different classes recomputed by the oracle here (the whole file: the
    generator, minutes)."""
    for cls in ("dup_vk_sig_doubled", "cancel_vk_sum_infinity", "vk_xb_plus_p", "second_generator", "generator_zero"):
        c = next(c for c in fx.cases if c["class"] == cls)
        got = o.verify_multi_bytes(fx.pt(c["sig"]), fx.msgs[c["msg"]], [fx.pt(v) for v in c["vks"]], fx.gens[c["gen"]])
        assert got is c["expect"], c["name"]
    for a in fx.aggregates:
        assert o.g1_to_bytes(o.aggregate([o.g1_from_bytes(fx.pt(s)) for s in a["sigs"]])) == fx.pt(a["out"]), a["name"]


def test_hash_keygen_sign_match_fixture(hc, fx):
    """H(m) of every message (padding boundaries, each digest range, first point at candidate
    1..16 and later), [sk]g of every key -- 0, r and r + 1 included: the ladder's infinity and
    P + (-P) branches -- and every signature."""
    for m, rec in zip(fx.msgs, fx.messages):
        out = ctypes.create_string_buffer(128)
        hc.edv_host_bls_hash(m, U64(len(m)), out)
        assert out.raw == fx.pt(rec["h"]), rec["name"]
    for k in fx.keys:
        out = ctypes.create_string_buffer(128)
        hc.edv_host_bls_keygen(bytes.fromhex(k["sk"]), fx.gens[k["gen"]], out)
        assert out.raw == fx.pt(k["vk"]), k["name"]
    for s in fx.signatures:
        out = ctypes.create_string_buffer(128)
        m = fx.msgs[s["msg"]]
        hc.edv_host_bls_sign(bytes.fromhex(fx.keys[s["key"]]["sk"]), m, U64(len(m)), out)
        assert out.raw == fx.pt(s["sig"]), (fx.keys[s["key"]]["name"], s["msg"])


def test_every_case_through_the_program(hc, fx):
    """All verdict cases through the wave form's program on the CPU (verkeys summed by g2_add:
    [vk, vk] takes its doubling branch, [vk, -vk] the infinity one); never a redo."""
    bad = []
    for c in fx.cases:
        m = fx.msgs[c["msg"]]
        vks = b"".join(fx.pt(v) for v in c["vks"])
        got = hc.edv_host_bls_verify_program(fx.pt(c["sig"]), m, U64(len(m)), vks, U64(len(c["vks"])), fx.gens[c["gen"]])
        assert got != 2, c["name"]
        if (got == 1) != c["expect"]:
            bad.append((c["name"], got))
    assert not bad, bad


def test_single_verkey_cases_through_bls_check(hc, fx):
    """The single-verkey cases through bn254.h's own pairing check (the one-, two- and four-lane
    kernels' arithmetic)."""
    n = 0
    for c in fx.cases:
        if len(c["vks"]) != 1:
            continue
        m = fx.msgs[c["msg"]]
        got = hc.edv_host_bls_verify(fx.pt(c["sig"]), m, U64(len(m)), fx.pt(c["vks"][0]), fx.gens[c["gen"]])
        assert got == int(c["expect"]), c["name"]
        n += 1
    assert n >= 60


def test_aggregates(hc, fx):
    """g1_add over repeated, cancelling, infinite and off-curve terms."""
    for a in fx.aggregates:
        out = ctypes.create_string_buffer(128)
        hc.edv_host_bls_aggregate(b"".join(fx.pt(s) for s in a["sigs"]), U64(len(a["sigs"])), out)
        assert out.raw == fx.pt(a["out"]), a["name"]


@pytest.mark.parametrize("name", sorted(ec.FP_OPS))
def test_fp_primitives_at_boundaries(hc, name):
    ec.check_fp(hc.edv_host_bn_fp, name)


def test_signed_sums_every_mask(hc):
    """blsp_sum: every term count with every sign mask over sums at exact multiples of p."""
    lay = ec.Layout(hc.edv_host_blsp_layout)
    assert ec.build_lin_table(lay).run(hc.edv_host_blsp_exec) > 50000


def test_products_inverses_zero_checks(hc):
    lay = ec.Layout(hc.edv_host_blsp_layout)
    assert ec.build_mul_inv_zchk_table(lay).run(hc.edv_host_blsp_exec) > 3000


def test_exec_refuses_a_slot_past_the_table(hc):
    lay = ec.Layout(hc.edv_host_blsp_layout)
    t = ec.ExecTable(lay)
    t.lin([1, 2], 0)
    ops = (ctypes.c_uint32 * lay.op_words)(*t.ops[0])
    slots = (ctypes.c_uint32 * 16)()
    out = (ctypes.c_uint32 * 8)()
    assert hc.edv_host_blsp_exec(ops, U64(1), slots, U64(2), out, ctypes.create_string_buffer(1),
                                 (ctypes.c_uint32 * 1)()) == -1
