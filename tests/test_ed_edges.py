"""The tables of tests/ed_edge_common.py through the CPU twins of the Ed25519 device probe
(edv_host_ed_* of libedv_hostcheck.so: the calls of tests/native/ed_probe.hip's one-item-per-lane
kernels, csrc/ed_probe_ops.h, compiled for the CPU with the EDV_BOUND_CHECK assertions).  A table
input outside the contract of fe_mul / fe_sq aborts here, so every table input is inside it, and
a failure of tests/test_gpu_ed_probe.py alone is the device's.  The wave forms (csrc/fe_lanes.h,
csrc/small_lanes.h) are device only; their CPU reference is the model of
tests/test_fe_lanes_model.py, checked here against integers on the inputs the device gets."""
import ctypes

import pytest

import ed_edge_common as ec


@pytest.fixture(scope="module")
def twin(hostcheck):
    return ec.Probe(hostcheck, "edv_host_ed", wave=False)


def test_op_list_is_the_builds(twin):
    io = (ctypes.c_int * 2)()
    assert twin.lane_io(len(ec.LANE_OPS) - 1, io) == 0 and twin.lane_io(len(ec.LANE_OPS), io) == -1
    assert twin.lane_io(-1, io) == -1
    assert twin.lane_fn(len(ec.LANE_OPS), None, ctypes.c_uint64(0), None) == -1
    assert twin.base_w == 16  # the host build's base comb (Makefile: -DEDV_BASE_W=16)


@pytest.mark.parametrize("name", ec.FIELD_OPS)
def test_field_ops_at_class_bounds(twin, name):
    assert ec.check_field(twin, name) > 500


@pytest.mark.parametrize("name", ec.SCALAR_OPS)
def test_scalar_ops_at_edges(twin, name):
    assert ec.check_scalar(twin, name) > 1000


@pytest.mark.parametrize("name", ec.RECODE_OPS)
def test_recodings_reconstruct_the_scalar(twin, name):
    assert ec.check_recode(twin, name) > 1000


def test_frombytes_on_edge_encodings(twin):
    assert ec.check_frombytes(twin) > 4000


@pytest.mark.parametrize("name", ["has_small_order", "is_canonical_point"])
def test_point_predicates_on_blacklist_neighbours(twin, name):
    assert ec.check_predicates(twin, name) > 3500


@pytest.mark.parametrize("name", ec.GROUP_OPS)
def test_group_ops_on_every_pair(twin, name):
    assert ec.check_group(twin, name) >= 45


def test_chained_walk(twin):
    assert ec.check_walk(twin) == 200


@pytest.mark.parametrize("form", [0, 1], ids=["verify_phase_hash", "verify_phase_hash_units"])
def test_hash_phase_lengths_alignments_fills(twin, form):
    assert ec.check_hash(twin, form) > 400


def test_hash_refuses_the_wave_form_and_a_message_outside_its_buffer(twin):
    z = ctypes.c_uint64(0)
    assert twin.hash_fn(2, None, None, None, z, None, None, z, None, None) == -1
    one = (ctypes.c_uint64 * 1)(8)
    assert twin.hash_fn(0, bytes(64), bytes(32), bytes(16), ctypes.c_uint64(16), (ctypes.c_uint64 * 1)(9), one,
                        ctypes.c_uint64(1), None, None) == -1


def test_sig_slot_texts_cover_every_length_and_group_residue():
    """The cases of check_sig_slot: text lengths 64..88, so every residue of the 5-digit Horner
    groups (csrc/sig_slot.h), and every count of leading zero bytes."""
    lens = set(ec.sig_slot_text_lengths(ec.sig_slot_values()))
    assert lens == set(range(64, 89)) and {n % 5 for n in lens} == {0, 1, 2, 3, 4}


def test_sig_slot_decode(twin):
    assert ec.check_sig_slot(twin) > 3000


def test_lane_model_is_exact_on_the_device_tables():
    assert ec.check_model_exact() > 1000
