"""The work list's lane code (csrc/wire_once.h) on the CPU (libedv_hostcheck.so hc_wire_once,
every access asserted in bounds) against a Python dict: which item's verdict every item of a
scanned batch takes, in any arrival order, at the table's edges and past the probe bound."""
import random

import numpy as np
import pytest

from wire_list_double import (DEAD, GENERAL, KEYED, NO_ID, SKIP, Batch, WireListOracleEngine, adversarial_messages,
                              dict_oracle, twin_once)

SIG_A = bytes(range(1, 65))
SIG_B = bytes(range(101, 165))
MSG = b"identifier:L5AD5g65TDQr1PPHHRoiGf|operation:dest:abc|reqId:1500000000000001|type:1"


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def _hand_made():
    """By name: (items, kid_u, pads)."""
    kid = [3, NO_ID, SKIP, 7]  # a registered key, a general one, one skipped, another key
    out = {}
    # the same triple at other alignments in the buffer
    out["alignments"] = ([(SIG_A, MSG, 0, 0)] * 5 + [(SIG_A, MSG[:-1], 0, 0)], kid, [0, 1, 7, 8, 15, 3])
    out["equal signature"] = ([(SIG_A, MSG, 0, 0), (SIG_A, _flip(MSG, 0), 0, 0), (SIG_A, _flip(MSG, len(MSG) - 1), 0, 0),
                               (SIG_A, MSG + b"x", 0, 0), (SIG_A, MSG[:-1], 0, 0), (SIG_A, MSG, 0, 0),
                               (SIG_A, _flip(MSG, 0), 0, 0), (SIG_A, b"", 0, 0), (SIG_A, b"", 0, 0)], kid, [5, 0, 3, 1, 2, 9, 4, 0, 0])
    out["equal message"] = ([(SIG_A, MSG, 0, 0), (_flip(SIG_A, 0), MSG, 0, 0), (_flip(SIG_A, 63), MSG, 0, 0),
                             (SIG_A, MSG, 0, 0), (_flip(SIG_A, 63), MSG, 0, 0)], kid, [0, 2, 4, 6, 1])
    out["two identifiers"] = ([(SIG_A, MSG, 0, 0), (SIG_A, MSG, 0, 3), (SIG_A, MSG, 0, 0), (SIG_A, MSG, 0, 3),
                               (SIG_A, MSG, 0, 1), (SIG_A, MSG, 0, 1)], kid, None)
    # the earliest member of a set of copies is dead: status 1 (uidx = nu), or a SKIP identifier
    out["dead first"] = ([(SIG_A, MSG, 1, 4), (SIG_A, MSG, 0, 0), (SIG_A, MSG, 0, 0), (SIG_B, MSG, 0, 2), (SIG_B, MSG, 0, 2),
                          (SIG_B, MSG, 0, 3), (SIG_B, MSG, 0, 3), (SIG_A, MSG, 1, 4)], kid, [1, 0, 2, 0, 3, 0, 4, 0])
    r = random.Random(9)
    pool = [(SIG_A if k % 2 else SIG_B, MSG + bytes([k % 5]), 0, k % 4) for k in range(20)]
    out["interleaved"] = ([r.choice(pool) for _ in range(300)], kid, [r.randrange(16) for _ in range(300)])
    out["empty"] = ([], kid, None)
    return out


HAND_MADE = _hand_made()


def _orders(n):
    r = random.Random(n)
    shuffled = list(range(n))
    r.shuffle(shuffled)
    return {"identity": list(range(n)), "reversed": list(range(n))[::-1], "shuffled": shuffled}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
@pytest.mark.parametrize("order", ["identity", "reversed", "shuffled"])
def test_representatives_equal_the_dict_oracle(hostcheck, name, order):
    items, kid, pads = HAND_MADE[name]
    b = Batch(items, kid, pads)
    want_rep, want_grp = dict_oracle(*b.args())
    lanes, rep, grp, gave, run = twin_once(hostcheck, *b.args(), order=_orders(b.n)[order])
    assert grp.tolist() == want_grp
    assert rep.tolist() == want_rep
    assert gave == 0 and run < 128
    assert lanes == sum(1 for i in range(b.n) if want_grp[i] != DEAD and want_rep[i] == i)
    # without `once` every live item stands for itself
    lanes0, rep0, grp0, _, run0 = twin_once(hostcheck, *b.args(), once=False)
    assert rep0.tolist() == list(range(b.n)) and grp0.tolist() == want_grp and run0 == 0
    assert lanes0 == sum(1 for g in want_grp if g != DEAD)


def test_the_hand_made_batches_hold_what_they_claim():
    rep, grp = dict_oracle(*Batch(*HAND_MADE["alignments"]).args())
    assert rep == [0, 0, 0, 0, 0, 5]
    rep, _ = dict_oracle(*Batch(*HAND_MADE["equal signature"]).args())
    assert rep == [0, 1, 2, 3, 4, 0, 1, 7, 7]
    rep, _ = dict_oracle(*Batch(*HAND_MADE["equal message"]).args())
    assert rep == [0, 1, 2, 0, 2]
    rep, grp = dict_oracle(*Batch(*HAND_MADE["two identifiers"]).args())
    assert rep == [0, 1, 0, 1, 4, 4] and grp == [KEYED, KEYED, KEYED, KEYED, GENERAL, GENERAL]
    rep, grp = dict_oracle(*Batch(*HAND_MADE["dead first"]).args())
    assert rep == [0, 1, 1, 3, 4, 5, 5, 7] and grp == [DEAD, KEYED, KEYED, DEAD, DEAD, KEYED, KEYED, DEAD]
    _, grp = dict_oracle(*Batch(*HAND_MADE["interleaved"]).args())
    assert {KEYED, GENERAL, DEAD} == set(grp)


def test_a_full_table_whose_chains_wrap(hostcheck):
    """cap = the number of distinct live triples: every slot taken, chains around the end."""
    items = [(SIG_A, MSG + bytes([k % 16]), 0, 0) for k in range(64)]
    b = Batch(items, [5], [k % 9 for k in range(64)])
    want_rep, _ = dict_oracle(*b.args())
    assert len(set(want_rep)) == 16
    for order in _orders(b.n).values():
        lanes, rep, _, gave, run = twin_once(hostcheck, *b.args(), cap=16, probe=16, order=order)
        assert rep.tolist() == want_rep and lanes == 16 and gave == 0 and run == 16


def _home(sig, uidx, length, cap):
    """csrc/wire_once.h wo_hash & (cap - 1)."""
    mask = (1 << 64) - 1
    h = 0xcbf29ce484222325 ^ (uidx << 32 | length)
    for k in range(16):
        h = ((h ^ int.from_bytes(sig[4 * k:4 * k + 4], "little")) * 0x100000001b3) & mask
    h ^= h >> 32
    h = (h * 0xd6e8feb86659fd93) & mask
    h ^= h >> 32
    return h & (cap - 1)


def test_a_home_slot_at_the_tables_end(hostcheck):
    """cap = 64, two triples whose home slot is 63 and one whose home is 0: the chain goes on
    around the table's end (slots 63, 0, 1)."""
    at_end = next(n for n in range(8, 4096) if _home(SIG_A, 0, n, 64) == 63)
    at_zero = next(n for n in range(8, 4096) if _home(SIG_A, 0, n, 64) == 0)
    x, x2, y = b"x" * at_end, b"x" * (at_end - 1) + b"y", b"z" * at_zero
    items = [(SIG_A, x, 0, 0), (SIG_A, x2, 0, 0), (SIG_A, y, 0, 0), (SIG_A, x2, 0, 0), (SIG_A, y, 0, 0), (SIG_A, x, 0, 0)]
    b = Batch(items, [5], [0, 1, 2, 3, 4, 5])
    for order in _orders(b.n).values():
        lanes, rep, _, gave, run = twin_once(hostcheck, *b.args(), cap=64, order=order)
        assert rep.tolist() == [0, 1, 2, 1, 2, 0] and lanes == 3 and gave == 0
        assert run == 3  # (counted around the end: 63, 0, 1)
    # the same three alone, one slot per probe: the second finds its home taken and gives up,
    # the third then finds slot 0 free -- the homes are where the model says
    three = Batch(items[:3], [5])
    assert twin_once(hostcheck, *three.args(), cap=64, probe=1)[3:] == (1, 2)
    assert twin_once(hostcheck, *three.args(), cap=64, probe=2)[3:] == (0, 3)
    assert twin_once(hostcheck, *three.args(), cap=128, probe=1)[3] <= 1


def test_the_probe_bound(hostcheck):
    """200 items of one identifier and one signature, pairwise different messages of one length:
    one hash (it covers the signature, the identifier and the length), so one home slot and one
    chain.  At bound 8 in 512 slots lanes give up and stand for themselves.  At bound 128 the
    chain grows to 128 slots and the other 72 give up: no bound below the batch's own size has
    no give-ups on 200 items of one home, whatever the table.  The batch's first 127 items are
    the longest such flood the device bound takes whole: run 127 < 128, no give-up."""
    msgs = adversarial_messages(200)
    assert len(set(msgs)) == 200 and len({len(m) for m in msgs}) == 1
    b = Batch([(SIG_A, m, 0, 0) for m in msgs], [0], [k % 8 for k in range(200)])
    lanes, rep, grp, gave, run = twin_once(hostcheck, *b.args(), cap=512, probe=8)
    # (equal signature, identifier and length: one home slot, a chain of 200)
    assert gave > 0 and run >= 200 - gave
    assert rep.tolist() == list(range(200)) and lanes == 200
    lanes, rep, _, gave, run = twin_once(hostcheck, *b.args(), cap=512, probe=128)
    assert rep.tolist() == list(range(200)) and lanes == 200
    assert gave == 200 - 128 and run == 128  # the chain is as long as the bound lets it grow
    b127 = Batch([(SIG_A, m, 0, 0) for m in msgs[:127]], [0], [k % 8 for k in range(127)])
    for order in _orders(127).values():
        lanes, rep, _, gave, run = twin_once(hostcheck, *b127.args(), cap=512, probe=128, order=order)
        assert (lanes, gave, run) == (127, 0, 127) and rep.tolist() == list(range(127))
    # copies of give-ups: each stands for itself, copies of placed items share
    items = [(SIG_A, m, 0, 0) for m in msgs] * 2
    b2 = Batch(items, [0])
    lanes, rep, _, gave, _ = twin_once(hostcheck, *b2.args(), cap=512, probe=8)
    want, _ = dict_oracle(*b2.args())
    assert gave > 0
    for i in range(400):
        assert rep[i] in (i, want[i])  # its own representative, or the true one
        assert rep[rep[i]] == rep[i]
    assert lanes == len({int(x) for x in rep})


def adversarial_texts(signer, count=200):
    """count request texts of one identifier with ONE signature over pairwise different requests
    of one serialized length (the signature is the first one's)."""
    import json

    import wire_model
    d = wire_model.nym_dict(random.Random(12), 0)
    d["identifier"] = signer.idr
    d["signature"] = wire_model.b58(signer.sign(d))
    return [json.dumps(dict(d, reqId=d["reqId"] + k)).encode() for k in range(count)]


def test_the_probe_bound_leaves_the_verdicts_unchanged(oracle, hostcheck):
    """The list double over the adversarial batch: bound 8 against bound 128 against wire_verify."""
    import wire_model
    from test_wire_authn import _Signer
    signer = _Signer(oracle, 1)
    buf, off = wire_model.pack_texts(adversarial_texts(signer))
    seen = {}
    for probe in (8, 128):
        eng = WireListOracleEngine(oracle, hostcheck)
        eng.once_cap, eng.once_probe = 512, probe
        first = eng.keys_add(np.frombuffer(signer.pk.raw, np.uint8).reshape(1, 32))
        status, _ = eng.wire_scan(buf, off)
        assert not status.any() and len(set(eng.wire[4].tolist())) == 1  # scanned; one message length
        uidx, uniq = eng.wire_idents()
        assert len(uniq) == 1
        ok, lanes = eng.wire_verify_list(np.array([first], np.uint32), None, True)
        assert ok.tolist() == eng.wire_verify(np.full(200, first, np.uint32)).tolist()
        assert ok.tolist() == [True] + [False] * 199
        seen[probe] = (lanes, eng.last_give_ups)
    assert seen[8][1] > 0 and seen[8][0] == 200
    assert seen[128] == (200, 200 - 128)


def test_bad_arguments(hostcheck):
    b = Batch([(SIG_A, MSG, 0, 0)], [5])
    assert twin_once(hostcheck, *b.args(), cap=48)[0] == -2
    sig, msgs, start, end, status, uidx, kid = b.args()
    assert twin_once(hostcheck, sig, msgs, start, [len(msgs) + 1], status, uidx, kid)[0] == -1
    assert twin_once(hostcheck, sig, msgs, [5], [4], status, uidx, kid)[0] == -1
