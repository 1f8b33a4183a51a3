"""The Ed25519 device arithmetic one primitive at a time against Python integers, through
libedv_ed_probe.so (tests/native/ed_probe.hip; test only).  Inside whole verifications these see
random-looking values and show only an accept bit; here the field code runs on limbs at the bounds
of the classes its callers pass (the device compiles the inline-asm v_mad_u64_u32 chains of
fe25519.h, the CPU twins of tests/test_ed_edges.py the C fallback), sc_reduce on values around
multiples of L and at its fold extremes, the decoders on the blacklist, the non-canonical and the
rootless encodings, the group operations on every pair of a set with torsion, P + P and P - P, and
the wave forms of the single-request kernels (csrc/fe_lanes.h, csrc/small_lanes.h) limb for limb
against the model of tests/test_fe_lanes_model.py, R's decode against the one-lane decoder, the
hash on the lanes at every pass edge and alignment, the tree sum at every lane position.  The
tables and references are tests/ed_edge_common.py's; a failure here alone is the device's.  Also
the signature slots' base58 decode (csrc/sig_slot.h) on every text length and leading-zero count,
and the general path's distinct-key dedupe (csrc/key_dedup.h) with the device's atomics against
the model of tests/dedup_cases.py."""
import ctypes
import os

import pytest

import dedup_cases as dc
import ed_edge_common as ec
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(gpu_engine):
    """The probe library, after the engine (and with it the one HIP runtime of the process)."""
    return ec.Probe(ctypes.CDLL(os.path.join(PKG, "libedv_ed_probe.so")), "edprobe", wave=True)


def test_op_lists_are_the_host_builds(probe, hostcheck):
    twin = ec.Probe(hostcheck, "edv_host_ed", wave=False)
    a, b = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    for op in range(len(ec.LANE_OPS)):
        assert probe.lane_io(op, a) == 0 and twin.lane_io(op, b) == 0 and list(a) == list(b)
    assert probe.lane_io(len(ec.LANE_OPS), a) == -1 and probe.wave_io(len(ec.WAVE_OPS), a) == -1
    assert probe.wave_io(len(ec.WAVE_OPS) - 1, a) == 0
    z = ctypes.c_uint64(0)
    assert probe.lane_fn(len(ec.LANE_OPS), None, z, None) == -1
    assert probe.wave_fn(len(ec.WAVE_OPS), None, ctypes.c_uint32(0), z, None) == -1
    assert probe.wave_fn(ec.WOP["tree_sum"], None, ctypes.c_uint32(48), z, None) == -1
    assert probe.hash_fn(3, None, None, None, z, None, None, z, None, None) == -1
    assert probe.base_w == 24


@pytest.mark.parametrize("name", ec.FIELD_OPS)
def test_field_ops_at_class_bounds(probe, name):
    assert ec.check_field(probe, name) > 500


@pytest.mark.parametrize("name", ec.SCALAR_OPS)
def test_scalar_ops_at_edges(probe, name):
    assert ec.check_scalar(probe, name) > 1000


@pytest.mark.parametrize("name", ec.RECODE_OPS)
def test_recodings_reconstruct_the_scalar(probe, name):
    assert ec.check_recode(probe, name) > 1000


def test_frombytes_on_edge_encodings(probe):
    assert ec.check_frombytes(probe) > 4000


@pytest.mark.parametrize("name", ["has_small_order", "is_canonical_point"])
def test_point_predicates_on_blacklist_neighbours(probe, name):
    assert ec.check_predicates(probe, name) > 3500


@pytest.mark.parametrize("name", ec.GROUP_OPS)
def test_group_ops_on_every_pair(probe, name):
    assert ec.check_group(probe, name) >= 45


def test_chained_walk(probe):
    assert ec.check_walk(probe) == 200


@pytest.mark.parametrize("form", [0, 1, 2],
                         ids=["verify_phase_hash", "verify_phase_hash_units", "verify_phase_hash_lanes"])
def test_hash_phase_lengths_alignments_fills(probe, form):
    assert ec.check_hash(probe, form) > 400


@pytest.mark.parametrize("name", ["dist_sq", "dist_mul", "dist_sqn", "cols_carry"])
def test_lane_forms_equal_the_model_limb_for_limb(probe, name):
    assert ec.check_dist(probe, name) > 600


def test_lane_form_chains_of_60_mixed_steps(probe):
    assert ec.check_dist_chains(probe) == 2400


def test_lane_form_round_trip(probe):
    assert ec.check_dist_round(probe) > 80


def test_r_decode_on_lanes_equals_the_one_lane_decoder(probe):
    assert ec.check_r_decode(probe) > 2000


@pytest.mark.parametrize("width", [16, 32, 64])
def test_tree_sum(probe, width):
    assert ec.check_tree_sum(probe, width) > 2 * width


def test_sig_slot_decode(probe):
    assert ec.check_sig_slot(probe) > 3000


@pytest.fixture(scope="module")
def dedup(gpu_engine):
    return dc.Dedup(ctypes.CDLL(os.path.join(PKG, "libedv_ed_probe.so")), "edprobe")


@pytest.fixture(scope="module")
def dedup_twin(hostcheck):
    return dc.Dedup(hostcheck, "edv_host_ed")


def test_dedup_entry_refuses_without_a_launch(dedup):
    k = [bytes(32)]
    assert dedup.call([], 16)[0] == -1 and dedup.call(k * 8, 7)[0] == -1 and dedup.call(k * 4097, 8194)[0] == -1


def test_dedup_multisets_meet_the_model(dedup, dedup_twin):
    """The cases of tests/test_key_dedup.py with the device's atomics: the model's invariants (the
    order of the inserts is free), and key_hash word for word the twin's."""
    for name, keys, nslots in dc.multiset_cases():
        r = dedup.run(keys, nslots)
        dc.check_model(keys, r, nslots)
        assert (r.hashes == dedup_twin.run(keys, nslots).hashes).all(), name


def test_dedup_wrap_and_chain_families(dedup, dedup_twin):
    pool = dc.family_pool()
    want = dedup_twin.hashes(pool)
    assert dedup.hashes(pool) == want
    dc.check_families(dedup, want)


def test_dedup_keys_one_word_apart_on_one_home_slot(dedup, dedup_twin):
    dc.check_near_twins(dedup, dedup_twin.hashes)


@pytest.mark.parametrize("word", [4, 6])
def test_dedup_counter_family_spreads(dedup, dedup_twin, word):
    keys = dc.counter_family(word)
    r = dedup.run(keys, 2 * len(keys))
    dc.check_model(keys, r, 2 * len(keys))
    assert (r.hashes == dedup_twin.run(keys, 2 * len(keys)).hashes).all()
    assert dc.displacement(keys, r, 2 * len(keys)) <= len(keys)
