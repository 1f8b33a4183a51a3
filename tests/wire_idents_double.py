"""WireOracleEngine with the engine's identifier pass (supports_wire_idents, wire_idents,
wire_verify_idents): the pass is the CPU twin of the kernels' lane code (libedv_hostcheck.so
hc_wire_idents, csrc/wire_idents.h), the verdicts are wire_verify's over kid_u[uidx].  Also
the helpers the identifier tests share (twin_idents, minimal request texts)."""
import ctypes

import numpy as np

import wire_model
from wire_double import WireOracleEngine


def pow2_at_least(x):
    cap = 1
    while cap < x:
        cap *= 2
    return cap


def twin_idents(lib, buf, off, status, span, cap=None, order=None):
    """hc_wire_idents: (nu, uidx[n], uniq_item[nu]); nu < 0 is the twin's error code.  cap
    defaults to the device's choice (a power of two >= 2 n), order to the identity."""
    n = len(off) - 1
    buf = np.ascontiguousarray(buf, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    status = np.ascontiguousarray(status, np.uint8)
    span = np.ascontiguousarray(span, np.uint32)
    order = np.ascontiguousarray(np.arange(n) if order is None else order, np.uint32)
    assert sorted(order.tolist()) == list(range(n))
    cap = pow2_at_least(max(64, 2 * n)) if cap is None else cap
    uidx = np.full(n, 0xDEADBEEF, np.uint32)
    uniq_item = np.full(n, 0xDEADBEEF, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.hc_wire_idents.restype = ctypes.c_int64
    nu = lib.hc_wire_idents(P(buf), P(off), ctypes.c_uint64(n), P(status), P(span), ctypes.c_uint64(cap), P(order),
                            P(uidx), P(uniq_item))
    return nu, uidx, uniq_item[:max(nu, 0)]


def ident_strings(buf, off, span, items):
    """The identifiers of `items` as the text holds them."""
    raw = np.asarray(buf, np.uint8).tobytes()
    return [raw[int(off[i]) + int(span[i, 0]):int(off[i]) + int(span[i, 0]) + int(span[i, 1])].decode("ascii")
            for i in np.asarray(items).tolist()]


_SIG = wire_model.b58(bytes(range(1, 65)))


def minimal_text(identifier, pad=0):
    """The smallest request text the scanner accepts with this identifier, `pad` spaces in
    front of it (the identifier at another alignment inside its text)."""
    return (" " * pad + '{"identifier":"%s","signature":"%s"}' % (identifier, _SIG)).encode()


def _hand_made():
    """Identifier sets in minimal request texts, by name."""
    sets = {
        "prefix pair": ["ab", "abc", "ab", "abc", "abc", "a", "ab"],
        "last byte": ["identifier-0", "identifier-1", "identifier-0", "identifier-2", "identifier-1"],
        "one byte": ["x", "y", "x", "idr", "y", "x"],
        "one identifier": ["L5AD5g65TDQr1PPHHRoiGf"] * 200,
        "only host items": None,
    }
    out = {k: [minimal_text(s) for s in v] for k, v in sets.items() if v is not None}
    out["alignments"] = [minimal_text("idr", pad) for pad in (0, 1, 2, 3, 0, 5, 8, 13)] + [minimal_text("idq", 1)]
    out["only host items"] = [b"{}", b"nul", b'{"identifier":"idr"}', b"", minimal_text("a\\nb")]
    return out


HAND_MADE = _hand_made()
HAND_NU = {"prefix pair": 3, "last byte": 3, "one byte": 3, "one identifier": 1, "only host items": 0, "alignments": 2}


class WireIdentsOracleEngine(WireOracleEngine):
    supports_wire_idents = True

    def __init__(self, lib=None, hostcheck=None):
        super().__init__(lib, hostcheck)
        self.wire_text = None
        self.wire_uidx = None
        self.wire_idents_calls = 0
        self.wire_verify_idents_calls = 0

    def wire_scan(self, text, text_off):
        status, span = super().wire_scan(text, text_off)
        text = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        self.wire_text = (text[:int(self.wire[0][-1])].copy(), span.copy())
        self.wire_uidx = None  # (the scan invalidates it)
        return status, span

    def wire_idents(self, out=None):
        if self.wire is None:
            raise RuntimeError("edverify error -1: no wire batch (edv_wire_scan first)")
        off, status = self.wire[0], self.wire[1]
        text, span = self.wire_text
        nu, uidx, uniq_item = twin_idents(self.hostcheck, text, off, status, span)
        assert nu >= 0, nu
        self.wire_uidx = (uidx, nu)
        self.wire_idents_calls += 1
        if out is None:
            return uidx.copy(), uniq_item.copy()
        view = np.frombuffer(out, np.uint32, count=len(uidx))  # (the engine writes the caller's buffer)
        view[:] = uidx
        return view, uniq_item.copy()

    def wire_verify_idents(self, kid_u):
        # edv_wire_verify_idents' preconditions
        assert self.wire is not None and self.wire_uidx is not None, "no identifier indices for this wire batch"
        uidx, nu = self.wire_uidx
        kid_u = np.asarray(kid_u, np.uint32)
        assert len(kid_u) == nu, (len(kid_u), nu)
        assert not self.wire[1].any(), "an item the host decides"
        assert (kid_u < self.WIRE_SKIP).all(), "an identifier without a key id"
        self.wire_verify_idents_calls += 1
        verifies = self.wire_verifies
        ok = self.wire_verify(kid_u[uidx] if len(uidx) else np.zeros(0, np.uint32))
        self.wire_verifies = verifies  # (counts the authenticator's own wire_verify calls)
        return ok
