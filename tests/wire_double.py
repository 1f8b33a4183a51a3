"""OracleEngine with the engine's wire interface (supports_wire, wire_scan, wire_verify,
wire_readback): the scan is the CPU twin of the kernel's lane code (libedv_hostcheck.so
hc_wire_scan), the verdicts are the C oracle's.  Host-side logic only, as engine_double."""
import ctypes
import os

import numpy as np

import wire_model
from engine_double import ROOT, OracleEngine


def load_hostcheck():
    return ctypes.CDLL(os.path.join(ROOT, "indy-plenum_amd", "libedv_hostcheck.so"))


class WireOracleEngine(OracleEngine):
    supports_wire = True
    WIRE_NO_ID = 0xFFFFFFFF
    WIRE_SKIP = 0xFFFFFFFE

    def __init__(self, lib=None, hostcheck=None):
        super().__init__(lib)
        self.hostcheck = hostcheck or load_hostcheck()
        self.wire = None
        self.wire_scans = 0
        self.wire_verifies = 0

    def wire_scan(self, text, text_off):
        text = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        off = np.array(text_off, np.uint64)
        status, span, sig, msgs, mlen = wire_model.twin_scan(self.hostcheck, text, off)
        self.wire = (off, status, sig, msgs, mlen)
        self.wire_scans += 1
        return status.copy(), span

    def wire_readback(self):
        assert self.wire is not None, "edverify error -1: no wire batch"
        _, _, sig, msgs, mlen = self.wire
        return sig.copy(), msgs[:int(self.wire[0][-1] - self.wire[0][0])].copy(), mlen.copy()

    def wire_verify(self, key_id, pk32=None):
        if self.wire is None:
            raise RuntimeError("edverify error -1: no wire batch (edv_wire_scan first)")
        off, status, sig, msgs, mlen = self.wire
        key_id = np.asarray(key_id, np.uint32)
        n = len(status)
        assert len(key_id) == n
        self.wire_verifies += 1
        ok = np.zeros(n, bool)
        live = status == 0
        for keyed in (True, False):
            sel = np.flatnonzero(live & ((key_id < self.WIRE_SKIP) if keyed else (key_id == self.WIRE_NO_ID)))
            if not len(sel):
                continue
            parts = [msgs[int(off[i] - off[0]):int(off[i] - off[0]) + int(mlen[i])].tobytes() for i in sel]
            o = np.zeros(len(sel) + 1, np.uint64)
            o[1:] = np.cumsum([len(p) for p in parts])
            buf = np.frombuffer(b"".join(parts), np.uint8)
            if keyed:
                ok[sel] = self.verify_batch_keyed(sig[sel], key_id[sel], buf, o)
            else:
                ok[sel] = self.verify_batch(sig[sel], np.asarray(pk32, np.uint8).reshape(-1, 32)[sel], buf, o)
        return ok
