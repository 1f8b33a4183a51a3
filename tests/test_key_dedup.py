"""The general path's distinct-key dedupe (csrc/key_dedup.h) through its CPU twin
edv_host_ed_dedup (libedv_hostcheck.so: the bodies of edv_dedup_insert_kernel and
edv_dedup_assign_kernel with the requests taken one after the other), against the model of
tests/dedup_cases.py: the distinct count, one representative per key, every request on its own
key's slot, the probe invariant, the split K and K * count <= n -- what the table region of a
sub-batch relies on and what verdicts cannot show.  tests/test_gpu_ed_probe.py runs the same
cases with the device's atomics."""
import random

import pytest

import dedup_cases as dc


@pytest.fixture(scope="module")
def twin(hostcheck):
    return dc.Dedup(hostcheck, "edv_host_ed")


@pytest.fixture(scope="module")
def cases():
    return dc.multiset_cases()


def test_entry_refuses_what_the_product_never_forms(twin):
    k = [bytes(32)]
    assert twin.call([], 16)[0] == -1          # no request
    assert twin.call(k * 8, 7)[0] == -1        # the table could fill up
    assert twin.call(k * 4097, 8194)[0] == -1  # more than 4096 requests
    assert twin.call(k * 8, 8)[0] == 0 and twin.call(k * 4096, 8192)[0] == 0


def test_case_list_has_the_exact_fits(cases):
    names = [c[0] for c in cases]
    for want in ("equal-1", "distinct-1024", "alternating-2", "c4-of-64", "c5-of-64", "c16-of-64", "c17-of-64",
                 "c64-of-1024", "c65-of-1024", "c256-of-1024", "c257-of-1024"):
        assert want in names
    splits = {name: dc.split_ref(len(set(keys)), len(keys)) for name, keys, _ in cases}
    assert (splits["c64-of-1024"], splits["c65-of-1024"], splits["c256-of-1024"], splits["c257-of-1024"]) == (8, 4, 4, 1)
    assert all(nslots == 2 * len(keys) for _, keys, nslots in cases)


def test_multisets_meet_the_model(twin, cases):
    for name, keys, nslots in cases:
        dc.check_model(keys, twin.run(keys, nslots), nslots)


def test_wrap_and_chain_families(twin):
    dc.check_families(twin)


def test_keys_one_word_apart_on_one_home_slot(twin):
    dc.check_near_twins(twin, twin.hashes)


def test_key_hash_is_the_python_restatement(twin):
    rng = random.Random(82)
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(1000)]
    assert twin.hashes(keys) == [dc.key_hash(k) for k in keys]


def test_every_key_byte_counts(twin):
    """The 256 keys that differ in one byte take 256 hash values, at each of the 32 positions: no
    word of a key is left out of its home slot."""
    base = bytes(random.Random(83).getrandbits(8) for _ in range(32))
    for pos in range(32):
        keys = [base[:pos] + bytes([b]) + base[pos + 1:] for b in range(256)]
        assert len(set(twin.hashes(keys))) == 256, pos


@pytest.mark.parametrize("word", [4, 6])
def test_counter_family_spreads(twin, word):
    """1,024 keys that differ in a counter in bytes 16..19 (24..27) at 2,048 slots: a total
    displacement of at most n.  Linear probing with uniform hashing at load 0.5 displaces 0.5 slots
    per key on average (Knuth: (1 + 1 / (1 - a)) / 2 probes), and n is twice that; a hash that
    leaves the word out puts all of them on one home slot, n (n - 1) / 2."""
    keys = dc.counter_family(word)
    r = twin.run(keys, 2 * len(keys))
    dc.check_model(keys, r, 2 * len(keys))
    assert dc.displacement(keys, r, 2 * len(keys)) <= len(keys)
