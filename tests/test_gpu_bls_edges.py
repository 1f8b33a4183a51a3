"""The BLS kernels (csrc/bls.hip) at their edges, bit for bit against the oracle's edge fixture
(tests/golden/bls_edge_vectors.json): scalars at the ends of the ladder, messages on SHA-256
padding boundaries and on H(m)'s try-and-increment edges, repeated and cancelling verkeys and
signatures, coordinates >= p, a second generator -- in every verify form (one wave per check,
four, two and one lane), at batch sizes around the 16-, 32- and 64-check verdict words, and
through the wave form's redo path with offsets that do not start at 0.
tests/test_bls_edges.py runs the same fixture through the CPU build of the same headers."""
import numpy as np
import pytest

import bls_edge_common as ec

pytestmark = pytest.mark.gpu

FORMS = ["wave", "quad", "pair", "one"]
SWEEP = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


def set_form(eng, form, n):
    """As tests/test_gpu_bls.py's bls_mode: selects the form for an n-check batch."""
    eng.bls_set_wave_checks(n if form == "wave" else 0)
    eng.bls_set_pair_lanes({"wave": 0, "quad": 2 * n, "pair": n, "one": 0}[form])


@pytest.fixture(scope="module")
def fx():
    return ec.fixture()


def _verify(eng, fx, cases, gen=0, **junk):
    sig, buf, off, vks, vk_off, want = ec.pack_cases(fx, cases, **junk)
    got = eng.bls_verify_batch(sig, buf, off, vks, np.frombuffer(fx.gens[gen], np.uint8), vk_off=vk_off)
    return got, want


def _assert_verdicts(got, want, cases, what):
    assert (got == want).all(), (what, [(i, c["name"]) for i, (c, g, w) in enumerate(zip(cases, got, want)) if g != w])


def test_fixture_conditions(fx):
    fx.check_conditions()


def test_keygen_sign_hash_match_oracle(gpu_engine, fx):
    """Every key (0, r and r + 1 included: outside the header's sk < r contract, they pin the
    ladder's infinity and P + (-P) branches), every signature, and H(m) of every message as
    [1]H(m)."""
    from plenum_amd import pack_messages
    assert {k["gen"] for k in fx.keys} == {0, 1, 4, 5}  # 4, 5: a twist point with x.a = 0, and written x.a = p
    for g in sorted({k["gen"] for k in fx.keys}):
        ks = [k for k in fx.keys if k["gen"] == g]
        sk = np.frombuffer(b"".join(bytes.fromhex(k["sk"]) for k in ks), np.uint8).reshape(-1, 32)
        got = gpu_engine.bls_keygen_batch(sk, np.frombuffer(fx.gens[g], np.uint8))
        want = fx.rows([k["vk"] for k in ks])
        assert (got == want).all(), [k["name"] for k, a, b in zip(ks, got, want) if (a != b).any()]
    sg = fx.signatures
    sk = np.frombuffer(b"".join(bytes.fromhex(fx.keys[s["key"]]["sk"]) for s in sg), np.uint8).reshape(-1, 32)
    buf, off = pack_messages([fx.msgs[s["msg"]] for s in sg])
    got = gpu_engine.bls_sign_batch(sk, buf, off)
    want = fx.rows([s["sig"] for s in sg])
    assert (got == want).all(), [(fx.keys[s["key"]]["name"], s["msg"]) for s, a, b in zip(sg, got, want) if (a != b).any()]
    one = np.zeros((len(fx.msgs), 32), np.uint8)
    one[:, 31] = 1
    buf, off = pack_messages(fx.msgs)
    got = gpu_engine.bls_sign_batch(one, buf, off)
    want = fx.rows([m["h"] for m in fx.messages])
    assert (got == want).all(), [m["name"] for m, a, b in zip(fx.messages, got, want) if (a != b).any()]


@pytest.mark.parametrize("form", FORMS)
def test_every_case_in_every_form(gpu_engine, fx, form):
    """One launch with all the cases over the reference generator -- finite, infinite, single and
    multi checks side by side in the waves and quads --, then one per other generator."""
    assert {c["gen"] for c in fx.cases} == {0, 1, 2, 3}
    for g in range(4):
        cases = [c for c in fx.cases if c["gen"] == g]
        set_form(gpu_engine, form, len(cases))
        got, want = _verify(gpu_engine, fx, cases, gen=g)
        _assert_verdicts(got, want, cases, (form, "generator %d" % g))


def test_aggregates_with_offset(gpu_engine, fx):
    """Every aggregate, sig_off[0] != 0: g1_add's doubling ([s, s]) and P + (-P) branches,
    infinite and off-curve terms, an empty range."""
    ag = fx.aggregates
    junk = 3
    sig_off = np.cumsum([junk] + [len(a["sigs"]) for a in ag]).astype(np.uint64)
    sigs = np.concatenate([np.full((junk, 128), 0x5A, np.uint8), fx.rows([s for a in ag for s in a["sigs"]])])
    out = gpu_engine.bls_aggregate(sigs, sig_off)
    want = fx.rows([a["out"] for a in ag])
    assert (out == want).all(), [a["name"] for a, x, y in zip(ag, out, want) if (x != y).any()]


@pytest.mark.parametrize("form", FORMS)
def test_shape_sweep(gpu_engine, fx, form):
    """Batches of n checks, check i = case (7 i + 3) mod m of the cases over the reference
    generator: partial last waves, the 16- and 32-bit verdict words, shuffles with dead partner
    lanes.  Then the same with a rejecting case forced at the first and last position of every
    16-check group (so of every 32- and 64-check group) and at the batch's last position."""
    main = ec.main_cases(fx)
    m = len(main)
    rej = [c for c in main if not c["expect"]]
    for n in SWEEP:
        plain = [main[(7 * i + 3) % m] for i in range(n)]
        forced = list(plain)
        for i in range(n):
            if i % 16 in (0, 15) or i == n - 1:
                forced[i] = rej[i % len(rej)]
        set_form(gpu_engine, form, n)
        for what, cases in (("plain", plain), ("forced", forced)):
            got, want = _verify(gpu_engine, fx, cases)
            _assert_verdicts(got, want, cases, (form, n, what))


@pytest.mark.parametrize("pair_lanes", [32768, 0])
@pytest.mark.parametrize("tries", [None, "16"])
def test_redo_path_with_offsets(gpu_engine, fx, monkeypatch, tries, pair_lanes):
    """The wave form hands over what it cannot decide (with EDV_BLS_HASH_TRIES=16: the messages
    whose first point is candidate 16 or later) and compacts those checks from the caller's
    arrays -- here with multi-signatures (vk_off) and with msg_off[0] != 0 and vk_off[0] != 0.
    The redo runs on the four-lane kernel, or with no pair lanes on the one-lane kernel."""
    if tries is None:
        monkeypatch.delenv("EDV_BLS_HASH_TRIES", raising=False)
    else:
        monkeypatch.setenv("EDV_BLS_HASH_TRIES", tries)
    main = ec.main_cases(fx)
    special = set(fx.special.values())
    cases = [c for c in main if c["msg"] in special]
    assert {c["msg"] for c in cases} == special and any(len(c["vks"]) == 25 for c in cases)
    cases = main[:3] + cases + [c for c in main if c["class"] in ("dup_vk_sig_doubled", "cancel_vk_sum_infinity",
                                                                   "cancel_vk_plus_third", "vk_xa_plus_p")]
    cases = cases[::2] + cases[1::2]  # the undecided checks apart from each other
    gpu_engine.bls_set_wave_checks(len(cases))
    gpu_engine.bls_set_pair_lanes(pair_lanes)
    got, want = _verify(gpu_engine, fx, cases, junk_msg=b"junk before the first message", junk_vk=5)
    _assert_verdicts(got, want, cases, (tries, pair_lanes))
    assert want.any() and not want.all()


def test_decreasing_offsets_are_refused(gpu_engine, fx):
    """EDV_EINVAL (-1) for a decreasing msg_off, vk_off or sig_off; the context verifies
    correctly afterwards."""
    from plenum_amd import EdVerifyError
    cases = ec.main_cases(fx)[:6]
    sig, buf, off, vks, vk_off, want = ec.pack_cases(fx, cases)
    gen = np.frombuffer(fx.gens[0], np.uint8)
    bad = off.copy()
    bad[2], bad[3] = off[3], off[2]
    assert bad[3] < bad[2]
    with pytest.raises(EdVerifyError) as e:
        gpu_engine.bls_verify_batch(sig, buf, bad, vks, gen, vk_off=vk_off)
    assert e.value.code == -1
    bad = vk_off.copy()
    bad[1] = vk_off[2] + 1
    assert bad[2] < bad[1]
    with pytest.raises(EdVerifyError) as e:
        gpu_engine.bls_verify_batch(sig, buf, off, vks, gen, vk_off=bad)
    assert e.value.code == -1
    with pytest.raises(EdVerifyError) as e:
        gpu_engine.bls_aggregate(sig, np.array([0, 4, 2, 6], np.uint64))
    assert e.value.code == -1
    got = gpu_engine.bls_verify_batch(sig, buf, off, vks, gen, vk_off=vk_off)
    _assert_verdicts(got, want, cases, "after the refusals")
    assert want.any()
