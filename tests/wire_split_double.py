"""WireNodeOracleEngine with the engine's entry interface (supports_wire_split,
wire_scan_entries, wire_raw_readback): the split is the CPU twin of the kernels' lane code
(libedv_hostcheck.so hc_node_split_lanes, csrc/node_split_lanes.h as an emulated wave), the
bodies are taken out of the entries at `at` as edv_node_copy_kernel does, and the unwrap, the
scan, the identifier pass and the verdicts are wire_node_double's over them."""
import numpy as np

import node_split_cases as nsc
from wire_node_double import WireNodeOracleEngine


class WireSplitOracleEngine(WireNodeOracleEngine):
    supports_wire_split = True

    def __init__(self, lib=None, hostcheck=None):
        super().__init__(lib, hostcheck)
        self.entry_scans = 0
        self.wire_raw = None

    def wire_scan_entries(self, text, entry_off):
        text = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else text
        entry_off = np.array(entry_off, np.uint64)
        assert int(entry_off[-1]) <= len(text)
        off, esc, entry, at = nsc.twin_split(self.hostcheck, text, entry_off)
        self.wire_raw = nsc.bodies_at(text, off, at)
        self.entry_scans += 1
        if len(esc) == 0:
            self.wire = None
            return (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, 2), np.uint32), esc, entry, at, off)
        scans = self.node_scans
        cls, status, span = self.wire_scan_node(self.wire_raw, off, esc)
        self.node_scans = scans  # (counts the authenticator's own wire_scan_node calls)
        return cls, status, span, esc, entry, at, off

    def wire_raw_readback(self):
        return self.wire_raw.copy()
