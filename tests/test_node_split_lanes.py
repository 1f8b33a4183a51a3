"""The device BATCH split's lane code on the CPU (libedv_hostcheck.so hc_node_split_lanes: the
functions of csrc/node_split_lanes.h as an emulated wave, every access asserted in bounds)
against the host split (_hostpack.gather_node_texts, csrc/node_split.h): the same verdict for
every entry and the same member spans, over the corpus, the boundary sweep and the member counts
of node_split_cases."""
import random

import numpy as np
import pytest

import node_split_cases as nsc


def _assert_equal(hostcheck, entries, base=0):
    text, eoff = nsc.pack(entries, base)
    off, esc, entry, at = nsc.twin_split(hostcheck, text, eoff)
    h_off, h_esc, h_entry, h_bodies = nsc.host_split(entries)
    assert off.tolist() == h_off.tolist()
    assert esc.tolist() == h_esc.tolist()
    assert entry.tolist() == h_entry.tolist()
    assert nsc.bodies_at(text, off, at).tobytes() == h_bodies.tobytes()
    # a whole entry starts where the entry does, a member inside its entry
    whole = esc == 0
    assert (at[whole] == eoff[entry[whole]]).all()
    assert (at[~whole] > eoff[entry[~whole]]).all()
    assert (at + np.diff(off) <= eoff[entry.astype(np.int64) + 1]).all()
    return esc, entry


def test_the_sweep_holds_both_verdicts():
    sweep = nsc.sweep_entries()
    _, esc, entry, _ = nsc.host_split(sweep)
    split = np.zeros(len(sweep), bool)
    split[entry[esc == 1]] = True
    assert split.sum() >= 1000 and (~split).sum() >= 1000
    assert len(entry) == len(sweep)  # one message each: the member, or the entry whole


@pytest.mark.parametrize("base", [0, 5])
def test_corpus_equals_the_host_split(hostcheck, base):
    esc, entry = _assert_equal(hostcheck, nsc.corpus_entries(), base)
    assert len(set(entry[esc == 1].tolist())) >= 10  # entries that split


def test_member_counts_equal_the_host_split(hostcheck):
    entries = nsc.count_entries()
    esc, entry = _assert_equal(hostcheck, entries)
    members = np.bincount(entry[esc == 1], minlength=len(entries)).tolist()
    assert {1, 2, 63, 64, 65, 70, 130} <= set(members)
    assert {1023, 1024, 1025} <= {len(e) for e in entries}


def test_boundary_sweep_equals_the_host_split(hostcheck):
    _assert_equal(hostcheck, nsc.sweep_entries())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shuffled_entries_at_every_alignment(hostcheck, seed):
    """The same entries at other alignments: shuffled, so each lies at another offset mod 16 and
    mod 1,024; an odd base."""
    r = random.Random(seed)
    pool = nsc.corpus_entries() + nsc.count_entries() + nsc.sweep_entries()[::7]
    _assert_equal(hostcheck, r.sample(pool, len(pool)), base=seed)


def test_no_entries_and_empty_entries(hostcheck):
    off, esc, entry, at = nsc.twin_split(hostcheck, np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert off.tolist() == [0] and len(esc) == len(entry) == len(at) == 0
    _assert_equal(hostcheck, [b"", b"", nsc.batch_of([]), b""])
