"""The drop-in against the reference's own classes, from the committed records.
tests/golden/check_dropin_ref.py mixes GpuAuthMixin in front of the reference's
SimpleAuthNr over the oracle-backed engine double and records the KAT outcomes,
engine-only verification (0 libsodium calls), the reference's BaseExc /
SuspiciousNode for a forged PROPAGATE (node.py:1313-1316) and 0 engine calls
for authenticate() after prefetch(); tests/golden/check_bls_dropin_ref.py does
the same for plenum_amd.bls over the reference's BLS ABCs and test scenarios.
Both need the reference's source tree, which is not part of this repository:
they are run by hand where it is, with --write, and the records they leave
(dropin_ref_check.json, bls_dropin_ref_check.json) are what is checked here."""
import json
import os

from conftest import GOLDEN


def test_committed_record():
    rec = json.load(open(os.path.join(GOLDEN, "dropin_ref_check.json")))
    assert rec["ok"] and rec["matched"] == rec["cases"] == 64
    assert rec["libsodium_crypto_sign_open_calls"] == 0
    assert rec["forged_propagate"].startswith("SuspiciousNode")
    # authenticate_batch == authenticate() over 5 signers on the reference class, before and after
    # a verkey is replaced, with the batch's keys from the native lookup (the reference's getVerkey)
    assert rec["batch_vs_single_matched"] == rec["batch_vs_single_items"] == 600
    assert rec["known_getverkey"] and rec["keys_known_native_calls"] == 2


def test_bls_committed_record():
    rec = json.load(open(os.path.join(GOLDEN, "bls_dropin_ref_check.json")))
    assert rec["ok"] and len(rec["checks"]) == 8
