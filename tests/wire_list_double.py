"""WireSplitOracleEngine with the engine's work-list verify (supports_wire_list,
wire_verify_list): the representatives are the CPU twin's of the kernels' lane code
(libedv_hostcheck.so hc_wire_once, csrc/wire_once.h), the verdicts are wire_verify's over the
representatives only, copied to the items they stand for.  Also the helpers the work-list tests
share (twin_once, the Python dict oracle, hand-made batches)."""
import ctypes

import numpy as np

from wire_idents_double import pow2_at_least
from wire_split_double import WireSplitOracleEngine

NO_ID = 0xFFFFFFFF
SKIP = 0xFFFFFFFE
DEAD, KEYED, GENERAL = 0, 1, 2
DEVICE_PROBE = 128  # csrc/wire_once.h kWireOnceProbe


def device_cap(n):
    """The table edv_wire_verify_list makes for n items."""
    return pow2_at_least(max(64, 2 * n))


def twin_once(lib, sig, msgs, start, end, status, uidx, kid_u, once=True, cap=None, probe=DEVICE_PROBE, order=None):
    """hc_wire_once: (lanes, rep[n], grp[n], give_ups, longest_run); lanes < 0 is the twin's
    error code.  cap defaults to the device's choice, order to the identity."""
    n = len(status)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1)
    msgs = np.ascontiguousarray(msgs, np.uint8)
    spans = np.ascontiguousarray(np.concatenate([np.asarray(start, np.uint64), np.asarray(end, np.uint64)]))
    status = np.ascontiguousarray(status, np.uint8)
    uidx = np.ascontiguousarray(uidx, np.uint32)
    kid_u = np.ascontiguousarray(kid_u, np.uint32)
    order = np.ascontiguousarray(np.arange(n) if order is None else order, np.uint32)
    assert sorted(order.tolist()) == list(range(n)) and len(sig) == 64 * n and len(uidx) == n
    cap = device_cap(n) if cap is None else cap
    rep = np.full(n, 0xDEADBEEF, np.uint32)
    grp = np.full(n, 0xEE, np.uint8)
    gave, run = ctypes.c_uint64(0), ctypes.c_uint64(0)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.hc_wire_once.restype = ctypes.c_int64
    lanes = lib.hc_wire_once(P(sig), P(msgs), ctypes.c_uint64(len(msgs)), P(spans), ctypes.c_uint64(n), P(status),
                             P(uidx), P(kid_u), ctypes.c_uint64(len(kid_u)), ctypes.c_uint32(1 if once else 0),
                             ctypes.c_uint64(cap), ctypes.c_uint32(probe), P(order), P(rep), P(grp),
                             ctypes.byref(gave), ctypes.byref(run))
    return lanes, rep, grp, gave.value, run.value


def dict_oracle(sig, msgs, start, end, status, uidx, kid_u):
    """(rep[n], grp[n]) by definition: item i is live iff status 0, an identifier and no SKIP;
    rep[i] = the smallest live j with the same (uidx, signature, message); a dead item's is itself."""
    n, nu = len(status), len(kid_u)
    sig = np.asarray(sig, np.uint8).reshape(n, 64)
    raw = np.asarray(msgs, np.uint8).tobytes()
    first, rep, grp = {}, [], []
    for i in range(n):
        live = status[i] == 0 and uidx[i] < nu and kid_u[uidx[i]] != SKIP
        grp.append(DEAD if not live else GENERAL if kid_u[uidx[i]] == NO_ID else KEYED)
        if not live:
            rep.append(i)
            continue
        key = (int(uidx[i]), sig[i].tobytes(), raw[int(start[i]):int(end[i])])
        rep.append(first.setdefault(key, i))
    return rep, grp


class Batch:
    """A hand-made scanned batch: items (sig64 bytes, message bytes, status, uidx) packed with
    `pad` filler bytes in front of each message (its alignment in the buffer)."""

    def __init__(self, items, kid_u, pads=None):
        n = len(items)
        pads = pads or [0] * n
        buf, self.start, self.end = bytearray(), [], []
        for (s, m, _, _), pad in zip(items, pads):
            buf += b"\xa5" * pad
            self.start.append(len(buf))
            buf += m
            self.end.append(len(buf))
        self.sig = np.frombuffer(b"".join(s for s, _, _, _ in items), np.uint8).reshape(n, 64)
        self.msgs = np.frombuffer(bytes(buf), np.uint8)
        self.status = np.array([st for _, _, st, _ in items], np.uint8)
        self.uidx = np.array([u for _, _, _, u in items], np.uint32)
        self.kid_u = np.array(kid_u, np.uint32)
        self.n = n

    def args(self):
        return self.sig, self.msgs, self.start, self.end, self.status, self.uidx, self.kid_u


def adversarial_messages(count=200, length=40):
    """Pairwise different messages of one length (for one identifier and one signature)."""
    return [b"m" * (length - 4) + i.to_bytes(4, "big") for i in range(count)]


class WireListOracleEngine(WireSplitOracleEngine):
    supports_wire_list = True

    def __init__(self, lib=None, hostcheck=None):
        super().__init__(lib, hostcheck)
        self.wire_list_calls = 0
        self.wire_list_lanes = 0
        self.once_cap = None      # the table's slots (default: the device's choice)
        self.once_probe = DEVICE_PROBE
        self.once_order = None    # a function n -> the order the live items are inserted in
        self.last_give_ups = 0

    def wire_verify_list(self, kid_u, pk_u=None, once=False):
        # edv_wire_verify_list's preconditions
        assert self.wire is not None and self.wire_uidx is not None, "no identifier indices for this wire batch"
        uidx, nu = self.wire_uidx
        kid_u = np.asarray(kid_u, np.uint32)
        assert len(kid_u) == nu, (len(kid_u), nu)
        assert pk_u is not None or not (kid_u == NO_ID).any(), "null pk_u with EDV_WIRE_NO_ID identifiers"
        off, status, sig, msgs, mlen = self.wire
        n = len(status)
        self.wire_list_calls += 1
        if n == 0:
            return np.zeros(0, bool), 0
        start = (off[:-1] - off[0]).astype(np.uint64)
        order = None if self.once_order is None else self.once_order(n)
        lanes, rep, grp, gave, _ = twin_once(self.hostcheck, sig, msgs, start, start + mlen, status, uidx, kid_u, once,
                                             self.once_cap, self.once_probe, order)
        assert lanes >= 0, lanes
        self.last_give_ups = gave
        mine = np.flatnonzero((grp != DEAD) & (rep == np.arange(n)))
        assert len(mine) == lanes
        key_id = np.full(n, SKIP, np.uint32)
        key_id[mine] = kid_u[uidx[mine]]
        pk32 = None
        if pk_u is not None:
            pk32 = np.zeros((n, 32), np.uint8)
            pk32[mine] = np.asarray(pk_u, np.uint8).reshape(-1, 32)[uidx[mine]]
        verifies = self.wire_verifies
        ok_rep = self.wire_verify(key_id, pk32)
        self.wire_verifies = verifies  # (counts the authenticator's own wire_verify calls)
        ok = ok_rep[rep] & (grp != DEAD)
        self.wire_list_lanes += lanes
        return ok, int(lanes)


def mixed_drain(dicts, nodes=3, members=70):
    """A node stack's drain over 3 + 3 * members signed request dicts: the first 3 as client
    texts; the others as `nodes` x 3 BATCHes of `members` PROPAGATEs, every node sending the same
    ones; 40 PREPARE / COMMIT texts, 22 as entries between the others and 2 as members of every
    BATCH; one member of the first BATCH with a \\u escape (the host decodes it)."""
    import json

    from plenum_amd.nodeloop import batch_text, propagate_text, three_phase_text
    assert len(dicts) == 3 + 3 * members
    props = [propagate_text(d, "client%d" % i) for i, d in enumerate(dicts)]
    phase = [three_phase_text("PREPARE" if k % 2 else "COMMIT", pp_seq_no=k + 1, bls_sig="s" * 20 if k % 4 == 0 else None)
             for k in range(40)]
    entries = [json.dumps(d) for d in dicts[:3]]
    used = 0
    for node in range(nodes):
        for b in range(3):
            m = props[3 + members * b:3 + members * (b + 1)]
            if node == 0 and b == 0:
                m = list(m)
                m[16] = m[16].replace("client19", "client\\u0031\\u0039")  # (request 19, the same message)
                assert "\\u" in m[16]
            entries.append(batch_text(m[:30] + [phase[used]] + m[30:] + [phase[used + 1]]))
            used += 2
    assert used == 2 * 3 * nodes
    rest = phase[used:]
    step = max(1, len(entries) // max(1, len(rest)))
    for k, t in enumerate(rest):  # (one in front of everything, the others spread over the drain)
        entries.insert(min(len(entries), k * (step + 1)), t)
    return [e.encode() for e in entries]
