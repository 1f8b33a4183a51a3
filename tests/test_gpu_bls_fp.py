"""The BLS wave form's Fp primitives on the device against Python integers:
fp_add / fp_sub / fp_neg / fp_dbl / fp_mul (bn254.h), the binary-gcd inverse fp_inv_plain_vt and
the program operations of blsp_exec -- the 9-limb signed sum blsp_sum with every term count and
sign mask, products of sums, inverses, zero checks (bls_wave.h) -- one item per lane through
libedv_bls_probe.so (tests/native/bls_fp_probe.hip; test only).  Inside whole pairings these
see random-looking values; here the operands sit on the boundaries: 0, p - 1, single limbs all
ones, sums at exact multiples of p.  The device compiles the __builtin_addc / __builtin_subc
chains, the CPU twins in tests/test_bls_edges.py the 64-bit fallback: a failure here alone is
the device's."""
import ctypes
import os

import pytest

import bls_edge_common as ec
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(gpu_engine):
    """The probe library, after the engine (and with it the one HIP runtime of the process)."""
    lib = ctypes.CDLL(os.path.join(PKG, "libedv_bls_probe.so"))
    lib.blsprobe_fp.restype = ctypes.c_int
    lib.blsprobe_exec.restype = ctypes.c_int
    return lib


def test_layout_is_the_host_builds(probe, hostcheck):
    a, b = ec.Layout(probe.blsprobe_layout), ec.Layout(hostcheck.edv_host_blsp_layout)
    assert vars(a) == vars(b)
    assert a.op_words >= 1 + (a.max_terms + 2) // 2


@pytest.mark.parametrize("name", sorted(ec.FP_OPS))
def test_fp_primitives_at_boundaries(probe, name):
    """All ordered pairs of ~40 boundary values and 4096 random pairs: (a +- b) mod p,
    a b 2^-256 mod p, a^(p-2) mod p with 0 -> 0."""
    ec.check_fp(probe.blsprobe_fp, name)


def test_signed_sums_every_mask(probe):
    """kLin: every term count 1..kMaxTerms with every sign mask over all p - 1, all 0, pairs
    x, p - x and sets summing to exactly p, 2p, 4p, 8p, each less one, and 12p - 12."""
    lay = ec.Layout(probe.blsprobe_layout)
    assert ec.build_lin_table(lay).run(probe.blsprobe_exec) > 50000


def test_products_inverses_zero_checks(probe):
    """kMul: sum_A sum_B 2^-256; kInv: s^-1 2^512; kZchk: the flag iff both slots are zero, and
    nothing written."""
    lay = ec.Layout(probe.blsprobe_layout)
    assert ec.build_mul_inv_zchk_table(lay).run(probe.blsprobe_exec) > 3000


def test_exec_refuses_a_slot_past_the_table(probe):
    lay = ec.Layout(probe.blsprobe_layout)
    t = ec.ExecTable(lay)
    t.lin([1, 2], 0)
    ops = (ctypes.c_uint32 * lay.op_words)(*t.ops[0])
    assert probe.blsprobe_exec(ops, ctypes.c_uint64(1), (ctypes.c_uint32 * 16)(), ctypes.c_uint64(2),
                               (ctypes.c_uint32 * 8)(), ctypes.create_string_buffer(1), (ctypes.c_uint32 * 1)()) == -1
