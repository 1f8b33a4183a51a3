"""bench.py without --full: the headline alone.  One small run (65,536
requests per batch, 64 signers): the line holds the whole-node figure for
exactly --steps timed batches and no other leg, every outcome is exact, and
--dump-outputs writes what the last timed authenticate_batch returned
(request i is signed by signer i % signers, all valid: the identifier of
signer i % 64 for every request)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_headline_alone(tmp_path):
    n, signers = 65536, 64
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--whole-node-n", str(n), "--signers", str(signers), "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-8000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith('{"metric')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "verifies/s" and d["higher_is_better"] is True
    w = d["whole_node"]
    s = w["synchronous"]
    assert w["batches"] == 3 and w["requests_per_batch"] == n
    assert d["ms_per_step"] == s["ms_per_batch"] > 0
    assert d["value"] == s["value"] and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert w["mismatches_all_ranks"] == 0 and d["parity"]["whole_node_mismatches"] == 0
    assert w["pipelined"] is None
    for leg in ("end_to_end", "device_resident", "roofline", "cpu_baseline", "tally", "collective", "whole_node_vs_cpu"):
        assert d[leg] is None, leg
    assert sorted(os.listdir(tmp_path / "out")) == ["whole_node_identifier_index.npy"]
    got = np.load(tmp_path / "out" / "whole_node_identifier_index.npy")
    assert got.dtype == np.float64 and got.shape == (n,)
    assert (got == np.arange(n) % signers).all()
