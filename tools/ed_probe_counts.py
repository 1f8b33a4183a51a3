"""Item counts and wall times of the Ed25519 probe checks (tests/ed_edge_common.py) on the device,
through libedv_ed_probe.so alone (test only; the package is not loaded):
    python tools/ed_probe_counts.py        # profiles/ed_probe/ed_counts.txt
Each line is one check_* call: table building, the launch and the comparison with Python integers."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "tests/golden", "indy-plenum_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))
import ed_edge_common as ec  # noqa: E402


def main():
    pr = ec.Probe(ctypes.CDLL(os.path.join(ROOT, "indy-plenum_amd", "libedv_ed_probe.so")), "edprobe", wave=True)

    def run(label, fn, *args):
        t = time.time()
        n = fn(pr, *args)
        print("%-32s %7d items %7.3f s" % (label, n, time.time() - t), flush=True)

    run("warm-up fe_add", ec.check_field, "fe_add")  # the first launch loads the code object
    for name in ec.FIELD_OPS:
        run(name, ec.check_field, name)
    for name in ec.SCALAR_OPS:
        run(name, ec.check_scalar, name)
    for name in ec.RECODE_OPS:
        run(name, ec.check_recode, name)
    run("ge_frombytes", ec.check_frombytes)
    for name in ("has_small_order", "is_canonical_point"):
        run(name, ec.check_predicates, name)
    for name in ec.GROUP_OPS:
        run(name, ec.check_group, name)
    run("walk", ec.check_walk)
    for form in (0, 1, 2):
        run("hash form %d" % form, ec.check_hash, form)
    for name in ("dist_sq", "dist_mul", "dist_sqn", "cols_carry"):
        run(name, ec.check_dist, name)
    run("dist chains", ec.check_dist_chains)
    run("dist round trip", ec.check_dist_round)
    run("r_decode", ec.check_r_decode)
    for width in (16, 32, 64):
        run("tree_sum %d" % width, ec.check_tree_sum, width)


if __name__ == "__main__":
    main()
