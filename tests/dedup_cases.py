"""Cases and the model of the general path's distinct-key dedupe (csrc/key_dedup.h: key_hash,
dedup_slot, the insert and the assign pass, split_of), shared by tests/test_key_dedup.py (the CPU
twin edv_host_ed_dedup of libedv_hostcheck.so, the requests one after the other) and
tests/test_gpu_ed_probe.py (edprobe_dedup of libedv_ed_probe.so: the product's kernels' bodies
with their atomics).  Which request represents a key and where a key lands in its probe chain
depend on the order of the inserts, so check_model asserts what holds in any order."""
import ctypes
import random

import numpy as np

EMPTY = 0xffffffff
_M = 0xffffffff
_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
SIZES = [1, 2, 63, 64, 65, 256, 257, 1024]


def key_hash(key):
    """csrc/key_dedup.h key_hash restated: every one of the eight little-endian key words counts"""
    w = [int.from_bytes(key[4 * k:4 * k + 4], "little") for k in range(8)]
    h = (w[0] * 0x9e3779b1) & _M
    h ^= (w[1] * 0x85ebca77) & _M
    h ^= ((w[2] ^ w[5]) * 0xc2b2ae3d) & _M
    h ^= ((w[3] ^ w[7]) * 0x27d4eb2f) & _M
    h ^= (w[4] * 0x165667b1) & _M
    h ^= (w[6] * 0xfd7046c5) & _M
    return h ^ (h >> 15)


def split_ref(count, n):
    return 8 if 16 * count <= n else 4 if 4 * count <= n else 1


class Result:
    pass


class Dedup:
    """The dedupe entry of one library: prefix "edprobe" (the device) or "edv_host_ed" (the twin)."""

    def __init__(self, lib, prefix):
        self.fn = getattr(lib, prefix + "_dedup")
        self.fn.restype = ctypes.c_int

    def call(self, keys, nslots):
        """the entry's return code and its outputs for the keys (a list of 32-byte strings)"""
        n = len(keys)
        pk = np.frombuffer(b"".join(keys) + bytes(32), np.uint8).copy()
        r = Result()
        r.slots, r.slot_u = np.zeros(max(nslots, 1), np.uint32), np.zeros(max(nslots, 1), np.uint32)
        r.req_slot, r.reps, r.hashes = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
        count, split = ctypes.c_uint32(0), ctypes.c_int(0)
        rc = self.fn(_P(pk.ctypes.data), _U64(n), _U64(nslots), _P(r.slots.ctypes.data), _P(r.req_slot.ctypes.data),
                     _P(r.slot_u.ctypes.data), _P(r.reps.ctypes.data), ctypes.byref(count), _P(r.hashes.ctypes.data),
                     ctypes.byref(split))
        r.count, r.split = count.value, split.value
        return rc, r

    def run(self, keys, nslots):
        rc, r = self.call(keys, nslots)
        assert rc == 0, rc
        return r

    def hashes(self, keys):
        """this build's key_hash of every key (in runs of distinct keys the entry takes)"""
        out = []
        for a in range(0, len(keys), 4096):
            out += [int(h) for h in self.run(keys[a:a + 4096], 8192).hashes[:len(keys[a:a + 4096])]]
        return out


def displacement(keys, r, nslots):
    """the sum over the occupied slots of the cyclic distance from the key's home slot"""
    return sum((h - int(r.hashes[s]) % nslots) % nslots for h, s in enumerate(r.slots.tolist()) if s != EMPTY)


def check_model(keys, r, nslots):
    n = len(keys)
    distinct = set(keys)
    count = r.count
    assert count == len(distinct), (count, len(distinct))
    reps = r.reps.tolist()
    assert all(u < n for u in reps[:count]) and {keys[u] for u in reps[:count]} == distinct  # one request per key
    assert all(u == EMPTY for u in reps[count:n])
    slots, slot_u, req_slot = r.slots.tolist(), r.slot_u.tolist(), r.req_slot.tolist()
    for i in range(n):
        s = req_slot[i]
        assert s < nslots and slots[s] < n and keys[slots[s]] == keys[i], (i, s)
        assert slot_u[s] < count and reps[slot_u[s]] == slots[s], (i, s, slot_u[s])
    occupied = [h for h in range(nslots) if slots[h] != EMPTY]
    assert len(occupied) == count
    assert all(slot_u[h] == EMPTY for h in range(nslots) if slots[h] == EMPTY)
    for h in occupied:  # the probe invariant: no empty slot between a key's home and its slot
        home = int(r.hashes[slots[h]]) % nslots
        d = (h - home) % nslots
        assert all(slots[(home + j) % nslots] != EMPTY for j in range(d)), (h, home)
    assert r.split == split_ref(count, n) and r.split * count <= n, (r.split, count, n)
    return occupied


def _keys(rng, c):
    out = set()
    while len(out) < c:
        out.add(bytes(rng.getrandbits(8) for _ in range(32)))
    return sorted(out)


def _uneven(rng, pool, n):
    """n requests over every key of the pool: each once, the rest drawn at random, shuffled"""
    ks = list(pool) + [pool[min(rng.randrange(len(pool)), rng.randrange(len(pool)))] for _ in range(n - len(pool))]
    rng.shuffle(ks)
    return ks


def multiset_cases():
    """(name, keys, nslots) with nslots = 2n: all equal, all distinct, two alternating, and c
    distinct keys at the two thresholds of split_of and one past each"""
    rng = random.Random(77)
    out = []
    for n in SIZES:
        pool = _keys(rng, n)
        out.append(("equal-%d" % n, [pool[0]] * n, 2 * n))
        out.append(("distinct-%d" % n, list(pool), 2 * n))
        if n >= 2:
            out.append(("alternating-%d" % n, [pool[i % 2] for i in range(n)], 2 * n))
        cs = ([n // 16, n // 16 + 1] if n % 16 == 0 else []) + ([n // 4, n // 4 + 1] if n % 4 == 0 else [])
        for c in cs:
            out.append(("c%d-of-%d" % (c, n), _uneven(rng, pool[:c], n), 2 * n))
    return out


FAMILY_POOL = 8192
FAMILY_SLOTS = 128


def family_pool():
    return _keys(random.Random(78), FAMILY_POOL)


def families(pool, hashes):
    """From a pool and its key_hash values: the wrap family (the keys whose home slot at 128 slots
    is the last one) and the chain family (the keys of the fullest other home slot)."""
    by_home = {}
    for k, h in zip(pool, hashes):
        by_home.setdefault(h % FAMILY_SLOTS, []).append(k)
    wrap = by_home.get(FAMILY_SLOTS - 1, [])
    chain_home = max((h for h in by_home if h < FAMILY_SLOTS - 1 - 48), key=lambda h: len(by_home[h]))
    return wrap, by_home[chain_home], chain_home


def wrap_batch(wrap):
    """32 keys of one home slot, 127 of 128: each twice, shuffled"""
    ks = wrap[:32] * 2
    random.Random(79).shuffle(ks)
    return ks


def chain_batch(chain):
    """48 keys of one home slot and 16 repeats, shuffled"""
    ks = chain[:48] + chain[:16]
    random.Random(80).shuffle(ks)
    return ks


def counter_family(word, n=1024):
    """n keys equal except for a little-endian counter in key word `word`"""
    base = _keys(random.Random(81 + word), 1)[0]
    return [base[:4 * word] + c.to_bytes(4, "little") + base[4 * word + 4:] for c in range(n)]


def near_twin_batch(hashes_of):
    """For each of the eight key words, 4 keys that differ in that word only and share a home slot
    at 128 slots (found with hashes_of, a build's key_hash), each twice, shuffled: 64 requests whose
    keys only the compare of all 32 bytes keeps apart."""
    rng = random.Random(84)
    ks = []
    for word in range(8):
        base = _keys(rng, 1)[0]
        cand = [base[:4 * word] + c.to_bytes(4, "little") + base[4 * word + 4:] for c in range(4096)]
        by_home = {}
        for k, h in zip(cand, hashes_of(cand)):
            by_home.setdefault(h % FAMILY_SLOTS, []).append(k)
        ks += next(v for v in by_home.values() if len(v) >= 4)[:4] * 2
    rng.shuffle(ks)
    return ks


def check_near_twins(dd, hashes_of):
    ks = near_twin_batch(hashes_of)
    r = dd.run(ks, FAMILY_SLOTS)
    check_model(ks, r, FAMILY_SLOTS)
    assert r.count == 32 and displacement(ks, r, FAMILY_SLOTS) >= 8 * 6  # each group of 4 walks 0 + 1 + 2 + 3


def check_families(dd, pool_hashes=None):
    """The wrap and the chain family through the dedupe dd, picked with pool_hashes (this build's
    key_hash of family_pool(); dd's own if not given)."""
    pool = family_pool()
    wrap, chain, chain_home = families(pool, pool_hashes if pool_hashes is not None else dd.hashes(pool))
    assert len(wrap) >= 32 and len(chain) >= 48, (len(wrap), len(chain))  # a uniform hash expects 64 per slot
    ks = wrap_batch(wrap)
    r = dd.run(ks, FAMILY_SLOTS)
    assert sorted(check_model(ks, r, FAMILY_SLOTS)) == list(range(31)) + [127]
    ks = chain_batch(chain)
    r = dd.run(ks, FAMILY_SLOTS)
    assert sorted(check_model(ks, r, FAMILY_SLOTS)) == list(range(chain_home, chain_home + 48))
    assert displacement(ks, r, FAMILY_SLOTS) == 48 * 47 // 2
