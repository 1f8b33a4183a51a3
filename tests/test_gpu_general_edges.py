"""The general path (any 32-byte key per request) through verify_batch at the edges of its
distinct-key dedupe (csrc/key_dedup.h): sub-batches whose distinct-key count sits on and just past
the thresholds of split_of -- K tables per key with K * count == n, the table region filled to
its last slot next to the following sub-batch's -- a ragged last sub-batch, and batches whose keys
all share one home slot of the hash table (a chain that wraps past the last slot, a chain of 48).
All messages are 40 bytes and the hash lanes unsorted, so the sub-batches are the pipeline's
quarters and last_launch_count() says so.  Expected verdicts follow from the construction (a
valid signature, 10% corrupted, one key per sub-batch that does not decode); a sample is checked
against the oracle."""
import ctypes

import numpy as np
import pytest

import dedup_cases as dc

pytestmark = pytest.mark.gpu
MLEN = 40


@pytest.fixture(scope="module")
def pool(gpu_engine, oracle):
    """300 keypairs and a 32-byte string that is no point"""
    rng = np.random.default_rng(90)
    pk, sk = gpu_engine.seed_keypair_batch(rng.integers(0, 256, (300, 32), dtype=np.uint8))
    out = ctypes.create_string_buffer(32)
    bad = next(k for k in (bytes([b]) + pk[0, 1:].tobytes() for b in range(256))
               if oracle.oracle_point_roundtrip(out, k) != 0)
    return pk, sk, np.frombuffer(bad, np.uint8)


class Sub:
    pass


def make_sub(eng, oracle, pool, seed, n, c):
    """n requests over c distinct keys (c - 1 of the pool and the one that does not decode), every
    key used, multiplicities uneven; 10% of the signatures corrupted; the first and last 64
    requests and every eighth checked against the oracle"""
    pk, sk, bad = pool
    rng = np.random.default_rng(seed)
    members = rng.choice(len(pk), c - 1, replace=False)
    which = np.concatenate([np.arange(c), np.minimum(rng.integers(0, c, n - c), rng.integers(0, c, n - c))])
    rng.shuffle(which)
    is_bad = which == c - 1
    kidx = np.where(is_bad, 0, members[np.minimum(which, c - 2)]).astype(np.uint32)
    s = Sub()
    s.n, s.c = n, c
    s.msgs = rng.integers(0, 256, n * MLEN, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * MLEN
    s.sig = eng.sign_batch(sk, kidx, s.msgs, off)
    s.pk = pk[kidx].copy()
    s.pk[is_bad] = bad
    assert len(np.unique(s.pk, axis=0)) == c
    corrupt = rng.random(n) < 0.1
    for i in np.nonzero(corrupt)[0]:
        s.sig[i, rng.integers(0, 64)] ^= 1 << int(rng.integers(0, 8))
    s.want = ~is_bad & ~corrupt
    assert s.want.any() and is_bad.any() and corrupt.any()
    for i in sorted(set(range(64)) | set(range(n - 64, n)) | set(range(0, n, 8))):
        m = s.msgs[i * MLEN:(i + 1) * MLEN].tobytes()
        assert (oracle.oracle_verify_detached(s.sig[i].tobytes(), m, MLEN, s.pk[i].tobytes()) == 0) == s.want[i], i
    return s


@pytest.fixture(scope="module")
def quarters(gpu_engine, oracle, pool):
    """sub-batches of 1,024 with 64 (K = 8 at its limit), 65 (K = 4 just past it), 256 (K = 4 filling
    all 1,024 table slots) and 257 (K = 1) distinct keys"""
    return [make_sub(gpu_engine, oracle, pool, 91 + j, 1024, c) for j, c in enumerate((64, 65, 256, 257))]


def run(eng, subs, pipeline):
    n = sum(s.n for s in subs)
    with eng.options(pipeline=pipeline, length_buckets=0):
        got = eng.verify_batch(np.concatenate([s.sig for s in subs]), np.concatenate([s.pk for s in subs]),
                               np.concatenate([s.msgs for s in subs]), np.arange(n + 1, dtype=np.uint64) * MLEN)
        launches, items = eng.last_launch_count(), eng.last_chunk_items()
    assert items == n
    return got, launches


def check(eng, subs):
    got, launches = run(eng, subs, 4)
    assert launches == 4
    want = np.concatenate([s.want for s in subs])
    assert (got == want).all(), np.nonzero(got != want)
    a = 0
    for s in subs:  # each sub-batch alone: the same bits
        alone, launches = run(eng, [s], 1)
        assert launches == 1 and (alone == got[a:a + s.n]).all()
        a += s.n


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0)], ids=["up", "down"])
def test_exact_fit_next_to_a_neighbour(gpu_engine, quarters, order):
    assert [dc.split_ref(s.c, s.n) for s in quarters] == [8, 4, 4, 1]
    assert [dc.split_ref(s.c, s.n) * s.c for s in quarters] == [512, 260, 1024, 257]
    check(gpu_engine, [quarters[j] for j in order])


@pytest.mark.parametrize("c", [255, 256])
def test_ragged_last_sub_batch(gpu_engine, oracle, pool, quarters, c):
    """3 * 1024 + 1023 requests: the last sub-batch has 1,023, with 255 distinct keys (4 * 255 <=
    1023: K = 4) and with 256 (K = 1)"""
    last = make_sub(gpu_engine, oracle, pool, 100 + c, 1023, c)
    assert dc.split_ref(c, 1023) == (4 if c == 255 else 1)
    check(gpu_engine, [quarters[2], quarters[0], quarters[3], last])


@pytest.fixture(scope="module")
def families(gpu_engine, hostcheck):
    """real keys picked with the host build's key_hash: 32 whose home slot of 128 is the last one, 48
    of one other home slot"""
    rng = np.random.default_rng(95)
    pk, sk = gpu_engine.seed_keypair_batch(rng.integers(0, 256, (dc.FAMILY_POOL, 32), dtype=np.uint8))
    keys = [k.tobytes() for k in pk]
    index = {k: i for i, k in enumerate(keys)}
    wrap, chain, _ = dc.families(keys, dc.Dedup(hostcheck, "edv_host_ed").hashes(keys))
    assert len(wrap) >= 32 and len(chain) >= 48, (len(wrap), len(chain))
    return pk, sk, [index[k] for k in dc.wrap_batch(wrap)], [index[k] for k in dc.chain_batch(chain)]


@pytest.mark.parametrize("family", ["wrap", "chain"])
def test_one_home_slot_through_the_product(gpu_engine, oracle, families, family):
    """64 requests (128 slots) whose keys share a home slot: 32 keys twice each on slot 127, so the
    chain runs on from slot 0; 48 keys and 16 repeats on one slot.  Verdicts equal the oracle's."""
    pk, sk, wrap, chain = families
    kidx = np.array(wrap if family == "wrap" else chain, np.uint32)
    assert len(kidx) == 64
    rng = np.random.default_rng(96)
    msgs = rng.integers(0, 256, 64 * MLEN, dtype=np.uint8)
    off = np.arange(65, dtype=np.uint64) * MLEN
    sig = gpu_engine.sign_batch(sk, kidx, msgs, off)
    sig[::5, 7] ^= 0x10
    sig[3::11, 40] ^= 0x01
    with gpu_engine.options(pipeline=1, length_buckets=0):
        got = gpu_engine.verify_batch(sig, pk[kidx], msgs, off)
        assert gpu_engine.last_launch_count() == 1 and gpu_engine.last_chunk_items() == 64
    want = np.array([oracle.oracle_verify_detached(sig[i].tobytes(), msgs[i * MLEN:(i + 1) * MLEN].tobytes(), MLEN,
                                                   pk[kidx[i]].tobytes()) == 0 for i in range(64)])
    assert (got == want).all() and want.sum() == 64 - len(set(range(0, 64, 5)) | set(range(3, 64, 11)))
