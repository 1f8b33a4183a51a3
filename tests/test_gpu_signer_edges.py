"""The device signer (edv_keypair_kernel, edv_sign_kernel) byte for byte against the oracle's
oracle_seed_keypair / oracle_sign_detached (oracle/ed25519_oracle.c: independent code, itself
checked against libsodium's vectors).  The nonce hash is sha512_prefixed<8> (a 32-byte prefix),
used nowhere else, with its padding edge at mlen = 79 mod 128; the hash over R || A || M has its
edge at 47 mod 128: every length around both edges up to 33 blocks is signed at all 16 message
alignments, every length 0..300 once, through key_idx onto shuffled key rows, over spans, behind
msg_off[0] != 0 and at the batch sizes around one block.  sign_batch makes the inputs of most GPU
tests here: a signer wrong at one (length, alignment) would otherwise show as a verify failure
somewhere else, or not at all.  Every signature made here also verifies under verify_batch, and
with byte 31, 32 or 63 flipped it does not."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEN_ALL = list(range(301))
LEN_EDGE = sorted({128 * b + e + d for b in range(1, 34) for e in (-81, -49) for d in (-1, 0, 1)
                   if 0 <= 128 * b + e + d <= 4200})
N_KEYS = 9


def oracle_keypair(oracle, seed):
    pk, sk = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_seed_keypair(pk, sk, bytes(seed))
    return pk.raw, sk.raw


def oracle_sign(oracle, msg, sk):
    sig = ctypes.create_string_buffer(64)
    oracle.oracle_sign_detached(sig, bytes(msg), ctypes.c_uint64(len(msg)), bytes(sk))
    return sig.raw


@pytest.fixture(scope="module")
def keys(oracle):
    """9 oracle keypairs and their sk64 rows in a shuffled order: (pk[9], sk[9], rows, row_of) with
    rows[row_of[k]] = sk[k]"""
    rng = np.random.default_rng(61)
    pairs = [oracle_keypair(oracle, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(N_KEYS)]
    pk = np.frombuffer(b"".join(p for p, _ in pairs), np.uint8).reshape(N_KEYS, 32)
    sk = np.frombuffer(b"".join(s for _, s in pairs), np.uint8).reshape(N_KEYS, 64)
    row_of = rng.permutation(N_KEYS)
    assert (row_of != np.arange(N_KEYS)).any()
    rows = np.zeros_like(sk)
    rows[row_of] = sk
    return pk, sk, rows, row_of


def _to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    return t


def sign_device(eng, rows, key_row, buf, off):
    """sign_batch_device on torch tensors: the message buffer on a 16-byte boundary with 16 spare
    bytes behind the last message, so off[i] mod 16 is message i's alignment"""
    import torch
    n = len(key_row)
    d_msgs = _to_dev(np.concatenate([np.asarray(buf, np.uint8), np.zeros(16, np.uint8)]))
    assert d_msgs.data_ptr() % 16 == 0
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=d_msgs.device)
    eng.sign_batch_device(_to_dev(rows), _to_dev(np.asarray(key_row, np.int32)), d_msgs,
                          _to_dev(np.asarray(off, np.uint64).view(np.int64)), n, d_sig)
    torch.cuda.synchronize()
    return d_sig.cpu().numpy()


def want_sigs(oracle, sk, key, msgs):
    return np.frombuffer(b"".join(oracle_sign(oracle, m, sk[k].tobytes()) for k, m in zip(key, msgs)),
                         np.uint8).reshape(len(msgs), 64)


def assert_sigs(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [what[i] for i in bad[:8]])


def check_verifier(eng, sig, pks, buf, off):
    """every signature verifies; with byte 31, 32 or 63 flipped none does"""
    assert eng.verify_batch(sig, pks, buf, off).all()
    for byte in (31, 32, 63):
        bad = sig.copy()
        bad[:, byte] ^= 1
        assert not eng.verify_batch(bad, pks, buf, off).any(), byte


def test_keypairs(gpu_engine, oracle):
    rng = np.random.default_rng(60)
    seeds = np.concatenate([rng.integers(0, 256, (254, 32), dtype=np.uint8), np.zeros((1, 32), np.uint8),
                            np.full((1, 32), 0xff, np.uint8), np.arange(32, dtype=np.uint8).reshape(1, 32)])
    assert seeds.shape == (257, 32)
    want = [oracle_keypair(oracle, s.tobytes()) for s in seeds]
    for n in (257, 1, 0):
        pk, sk = gpu_engine.seed_keypair_batch(seeds[:n])
        assert pk.shape == (n, 32) and sk.shape == (n, 64)
        for i in range(n):
            assert pk[i].tobytes() == want[i][0] and sk[i].tobytes() == want[i][1], (n, i)
            assert sk[i].tobytes() == seeds[i].tobytes() + pk[i].tobytes()


def test_every_length_to_300(gpu_engine, oracle, keys):
    pk, sk, rows, row_of = keys
    rng = np.random.default_rng(62)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LEN_ALL]
    key = rng.integers(0, N_KEYS, len(msgs))
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    got = sign_device(gpu_engine, rows, row_of[key], buf, off)
    assert_sigs(got, want_sigs(oracle, sk, key, msgs), [(len(m), int(o) % 16) for m, o in zip(msgs, off)])
    check_verifier(gpu_engine, got, pk[key], buf, off)


def edge_items():
    """Every LEN_EDGE length at every alignment, packed back to back: the next message is one of
    those still wanted at the alignment the buffer has reached, behind a pad of 1..15 bytes (an
    item of its own, signed and checked like any other) where there is none."""
    rng = np.random.default_rng(63)
    todo = {a: list(rng.permutation(LEN_EDGE)) for a in range(16)}
    lens, pos = [], 0
    while any(todo.values()):
        a = pos % 16
        if not todo[a]:
            pad = next(d for d in range(1, 16) if todo[(a + d) % 16])
            lens.append(pad)
            pos += pad
            continue
        lens.append(int(todo[a].pop()))
        pos += lens[-1]
    return lens


def test_pad_edges_at_every_alignment(gpu_engine, oracle, keys):
    pk, sk, rows, row_of = keys
    rng = np.random.default_rng(64)
    lens = edge_items()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert {(n, int(o) % 16) for n, o in zip(lens, off)} >= {(n, a) for n in LEN_EDGE for a in range(16)}
    assert len(LEN_EDGE) == 198 and len(lens) < 16 * len(LEN_EDGE) + 64
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    msgs = [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(lens))]
    key = rng.integers(0, N_KEYS, len(lens))
    got = sign_device(gpu_engine, rows, row_of[key], buf, off)
    assert_sigs(got, want_sigs(oracle, sk, key, msgs), [(n, int(o) % 16) for n, o in zip(lens, off)])
    check_verifier(gpu_engine, got, pk[key], buf, off)


def test_key_idx_picks_the_row(gpu_engine, oracle, keys):
    """key_idx with repeats onto shuffled rows: a wrong row gives a valid signature of another key"""
    pk, sk, rows, row_of = keys
    rng = np.random.default_rng(65)
    key = np.array([3, 3, 0, 8, 1, 8, 8, 2, 7, 6, 5, 4, 0, 3, 1, 7])
    assert (row_of[key] != np.arange(len(key))).any() and len(set(key)) == N_KEYS
    msgs = [rng.integers(0, 256, 40 + i, dtype=np.uint8).tobytes() for i in range(len(key))]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    want = want_sigs(oracle, sk, key, msgs)
    got = sign_device(gpu_engine, rows, row_of[key], buf, off)
    assert_sigs(got, want, list(key))
    assert_sigs(gpu_engine.sign_batch(rows, row_of[key], buf, off), want, list(key))
    check_verifier(gpu_engine, got, pk[key], buf, off)


def test_spans_over_one_copy(gpu_engine, oracle, keys):
    """sign_spans_device: 40 messages with junk between them, 1..5 signatures over each copy"""
    import torch
    pk, sk, rows, row_of = keys
    rng = np.random.default_rng(66)
    buf, start, end = bytearray(), [], []
    for r in range(40):
        buf += bytes(rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8))
        start.append(len(buf))
        buf += bytes(rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8))
        end.append(len(buf))
    item_req, key = [], []
    for r in rng.permutation(40):
        k = int(rng.integers(1, 6))
        item_req += [int(r)] * k
        key += list(rng.choice(N_KEYS, k, replace=False))
    key, n = np.array(key), len(key)
    ms, me = np.array(start, np.uint64)[item_req], np.array(end, np.uint64)[item_req]
    assert (ms[1:] != me[:-1]).any()
    msgs = [bytes(buf[int(a):int(b)]) for a, b in zip(ms, me)]
    d_msgs = _to_dev(np.concatenate([np.frombuffer(bytes(buf), np.uint8), np.zeros(16, np.uint8)]))
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=d_msgs.device)
    gpu_engine.sign_spans_device(_to_dev(rows), _to_dev(row_of[key].astype(np.int32)), d_msgs,
                                 _to_dev(ms.view(np.int64)), _to_dev(me.view(np.int64)), n, d_sig)
    torch.cuda.synchronize()
    got = d_sig.cpu().numpy()
    assert_sigs(got, want_sigs(oracle, sk, key, msgs), item_req)
    dbuf = np.frombuffer(b"".join(msgs), np.uint8)
    doff = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    check_verifier(gpu_engine, got, pk[key], dbuf, doff)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_batch_sizes_behind_a_first_offset_of_3(gpu_engine, oracle, keys, n):
    pk, sk, rows, row_of = keys
    rng = np.random.default_rng(67 + n)
    msgs = [rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8).tobytes() for _ in range(n)]
    key = rng.integers(0, N_KEYS, n)
    off = (3 + np.concatenate([[0], np.cumsum([len(m) for m in msgs])])).astype(np.uint64)
    buf = np.frombuffer(b"\xab\xcd\xef" + b"".join(msgs), np.uint8)
    want = want_sigs(oracle, sk, key, msgs)
    got = sign_device(gpu_engine, rows, row_of[key], buf, off)
    assert_sigs(got, want, list(range(n)))
    assert_sigs(gpu_engine.sign_batch(rows, row_of[key], buf, off), want, list(range(n)))
    check_verifier(gpu_engine, got, pk[key], buf, off)
