"""The wire doubles with the engine's digest pass (supports_wire_digests, wire_digests): the
pass is the CPU twin of the kernel's lane code (libedv_hostcheck.so hc_wire_digests,
csrc/wire_digest.h) over what the double's scan kept.  Also the helpers the digest tests
share: the rule in Python, the definition of a digest, the twin's entry points."""
import ctypes
import hashlib
import json

import numpy as np

from plenum_amd.request_digest import signing_state
from plenum_amd.serialization import serialize_msg_for_signing
from wire_double import WireOracleEngine
from wire_node_double import WireNodeOracleEngine

FIVE = {"identifier", "reqId", "operation", "protocolVersion", "signature"}


def eligible(d):
    """The rule: the bytes the signature covers are the signingState's bytes."""
    return (set(d) <= FIVE and "reqId" in d and "operation" in d
            and not ("protocolVersion" in d and d["protocolVersion"] is None))


def definition(d):
    """Request.digest of the request dict, as bytes."""
    return hashlib.sha256(serialize_msg_for_signing(signing_state(d))).digest()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def twin_eligible(lib, text):
    """hc_wd_eligible over exactly these bytes (every read asserted inside them)."""
    buf = np.frombuffer(bytes(text) + b"\xee" * 16, np.uint8)  # (what follows is not the item's)
    lib.hc_wd_eligible.restype = ctypes.c_uint32
    return int(lib.hc_wd_eligible(_p(buf), ctypes.c_uint64(0), ctypes.c_uint32(len(text))))


def twin_digests(lib, buf, off, status, msgs, mlen):
    """hc_wire_digests over packed texts and hc_wire_scan's results: (digest[n, 32], have bool[n])."""
    n = len(off) - 1
    buf = np.ascontiguousarray(buf, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    status = np.ascontiguousarray(status, np.uint8)
    msgs = np.ascontiguousarray(msgs, np.uint8)
    mlen = np.ascontiguousarray(mlen, np.uint32)
    dig = np.full((n, 32), 0xAB, np.uint8)
    have = np.full(n, 0xAB, np.uint8)
    lib.hc_wire_digests.restype = None
    lib.hc_wire_digests(_p(buf), _p(off), ctypes.c_uint64(n), _p(status), _p(msgs), _p(mlen), _p(dig), _p(have))
    assert set(np.unique(have).tolist()) <= {0, 1}
    return dig, have.astype(bool)


class _Digests:
    supports_wire_digests = True
    wire_digest_calls = 0

    def wire_scan(self, text, text_off):
        out = super().wire_scan(text, text_off)
        text = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        self.digest_text = text[:int(self.wire[0][-1])].copy()  # the text the scan read
        return out

    def wire_digests(self, out=None):
        if self.wire is None:
            raise RuntimeError("edverify error -1: no wire batch (edv_wire_scan first)")
        off, status, _, msgs, mlen = self.wire
        self.wire_digest_calls += 1
        return twin_digests(self.hostcheck, self.digest_text, off, status, msgs, mlen)


class WireDigestOracleEngine(_Digests, WireOracleEngine):
    pass


class WireDigestNodeOracleEngine(_Digests, WireNodeOracleEngine):
    pass


def check_contract(results, digest, have, decoded):
    """The triple against the definition: decoded[i] is result i's request dict (None where
    the text does not decode).  Returns the number of accepted items."""
    n = len(results)
    assert digest.shape == (n, 32) and digest.dtype == np.uint8
    assert have.shape == (n,) and have.dtype == bool
    for i, r in enumerate(results):
        accepted = not isinstance(r, Exception)
        assert bool(have[i]) == accepted, (i, r)
        if accepted:
            assert digest[i].tobytes() == definition(decoded[i]), (i, decoded[i])
        else:
            assert not digest[i].any(), i
    return int(have.sum())


def loads_or_none(text):
    try:
        return json.loads(text)
    except ValueError:
        return None
