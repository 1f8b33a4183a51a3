"""WireIdentsOracleEngine with the engine's node-message interface (supports_wire_node,
wire_scan_node, wire_ident_text): the unwrap is the CPU twin of the kernel's lane code
(libedv_hostcheck.so hc_wire_unwrap, csrc/wire_unwrap.h), and the scan, the identifier pass
and the verdicts then run over the unwrapped buffer as wire_idents_double's do over texts."""
import numpy as np

import wire_unwrap_model as wum
from wire_idents_double import WireIdentsOracleEngine, ident_strings


class WireNodeOracleEngine(WireIdentsOracleEngine):
    supports_wire_node = True
    NODE_REQUEST, NODE_HOST, NODE_NONE = 0, 1, 2

    def __init__(self, lib=None, hostcheck=None):
        super().__init__(lib, hostcheck)
        self.node_scans = 0
        self.ident_text_calls = 0

    def wire_scan_node(self, text, text_off, esc):
        text = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        off = np.array(text_off, np.uint64)
        assert len(esc) == len(off) - 1
        cls, unwrapped = wum.twin_unwrap(self.hostcheck, text[int(off[0]):int(off[-1])], off - off[0], esc)
        self.node_scans += 1
        # (the host's buffer is NOT what the scan read: the spans are relative to `unwrapped`)
        status, span = self.wire_scan(unwrapped, off - off[0])
        return cls, status, span

    def wire_ident_text(self, uniq_item):
        assert self.wire is not None and self.wire_text is not None
        self.ident_text_calls += 1
        text, span = self.wire_text
        assert not self.wire[1][np.asarray(uniq_item, np.int64)].any(), "not a scanned item"
        return [s.encode("ascii") for s in ident_strings(text, self.wire[0], span, uniq_item)]
