"""From the wire to a verdict, three ways, alternating in one process on one GPU:
  (a) authenticate_wire_batch(texts)   the request texts as received; scanned on the GPU
  (b) authenticate_batch(dicts)        the headline path over already-decoded dicts
  (c) json.loads per text + (b)        what a node pays today from the same texts
over configs[1]'s shape: n NYM requests (1M), 1,000 registered signers, rendered once to
wire texts.  Every timed batch's verdicts are checked for equality between the paths, and
the wire path must leave no item to the host.  Prints one JSON line: the three rates, the
p50 ms per batch, and the wire path's breakdown (gather, PCIe + scan kernel, key
resolution, verify, result list).

--idents-ab: path (a) alone, two ways alternating in one process: the batch's distinct identifiers
found on the GPU (EDV_WIRE_IDENTS=1: edv_wire_idents, edv_wire_verify_idents) and on the host
(EDV_WIRE_IDENTS=0: _hostpack.wire_idents); p50 and min-max of the `keys` phase and of the batch.

--node: a node stack's drain (nodeloop.drain_texts: per group of --members requests, one BATCH of
their PROPAGATEs from each of the other pool - 1 nodes), about --n signed requests in all, for a
4-node and a 25-node pool, four ways alternating in one process:
  (a) authenticate_node_wire_batch(entries), EDV_WIRE_SPLIT=0        split on the host, unwrapped and scanned on the GPU
  (a') the same with EDV_WIRE_SPLIT=1 (node_wire_split)              the entries copied whole, split on the GPU too
  (b) authenticate_batch(batching.requests_in_drain(entries))        what a node pays today
  (c) authenticate_wire_batch(the bare client texts, same requests)  the scan's own cost, no unwrap
with the results asserted equal in every batch; p50 and min-max per path and per phase of (a), (a') and (c).

--node --mixed: the --node drain as a running node sees it -- per group of --members requests and
per sending node one PREPARE and one COMMIT entry next to the BATCH (nodeloop.three_phase_text), so
no batch is all scanned requests -- three ways alternating in one process, on both pools:
  (p) EDV_WIRE_LIST=0                  per-item key ids built on the host, edv_wire_verify
  (l) EDV_WIRE_LIST=1                  one key per identifier, the work list built on the GPU (edv_wire_verify_list)
  (o) EDV_WIRE_ONCE=1                  (l), each distinct (identifier, signature, message) verified once
with the results asserted equal in every batch; p50 and min-max of the batch and of its phases.  Then
(l) and (o) over the bare client texts (authenticate_wire_batch, no copies: what `once` costs a
drain it cannot help).

--digests: path (a) with and without the request digests, and what a caller pays for them today,
alternating in one process:
  (plain)   authenticate_wire_batch(texts)                                    no digests
  (digests) authenticate_wire_batch(texts, digests=True)                      hashed on the GPU from the scan's bytes
  (today)   (plain), then json.loads of every accepted text + request_digests(dicts, engine)
with every digest asserted equal between the last two in every batch; p50 and min-max per leg and of
each leg's added time over (plain) in the same round.

usage: python tools/wire_probe.py [--n 1000000] [--signers 1000] [--batches 10] [--out FILE]
                                  [--idents-ab | --digests | --node [--mixed]]
       python tools/wire_probe.py --write-corpus FILE        (no GPU: the test corpora, length-prefixed,
       python tools/wire_probe.py --write-node-corpus FILE    for indy-plenum_amd/build/wire_corpus_check [--node])
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indy-plenum_amd"))


def write_corpus(path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wire_model
    texts = wire_model.corpus()
    with open(path, "wb") as f:
        for t in texts:
            f.write(struct.pack("<I", len(t)))
            f.write(t)
    print("wrote %d texts to %s" % (len(texts), path))


def write_node_corpus(path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wire_unwrap_model
    corp = wire_unwrap_model.corpus()
    entries = corp["clean"] + corp["mutated"]
    with open(path, "wb") as f:
        for t in entries:
            f.write(struct.pack("<I", len(t)))
            f.write(t)
    print("wrote %d entries to %s" % (len(entries), path))


def build(eng, n, signers, alias_len):
    """(texts, dicts, identifiers, verkeys): configs[1] NYM requests signed on the GPU."""
    import numpy as np
    from plenum_amd import _hostpack, pack_messages, synth
    from plenum_amd.base58 import b58encode
    pks, sks = eng.seed_keypair_batch(synth.signer_seeds(signers))
    msgs, kidx, spec = synth.nym_messages(n, pks, alias_len=alias_len, seed=1)
    buf, off = pack_messages(msgs)
    sig = eng.sign_batch(sks, kidx, buf, off)
    sig_b58 = _hostpack.b58encode_rows(np.ascontiguousarray(sig).tobytes(), 64)
    idrs, dests, vk_pool, pool, base = spec["idrs"], spec["dests"], spec["vks"], spec["pool"], spec["req_id_base"]
    alias = "" if spec["alias"] is None else ', "alias": "%s"' % spec["alias"]
    fmt = ('{"identifier": "%s", "reqId": %d, "operation": {"type": "1", "dest": "%s", "verkey": "%s"' + alias
           + '}, "protocolVersion": 1, "signature": "%s"}')
    first = synth.nym_request_dict(spec, 0, signers)
    first["signature"] = sig_b58[0]
    assert fmt % (idrs[0], base, dests[0], vk_pool[0], sig_b58[0]) == json.dumps(first)
    texts = [(fmt % (idrs[i % signers], base + i, dests[i % pool], vk_pool[(i * 7) % pool], sig_b58[i])).encode()
             for i in range(n)]
    dicts = [json.loads(t) for t in texts]
    return texts, dicts, idrs, ["~" + b58encode(bytes(pk[16:])) for pk in pks]


def idents_ab(eng, args, texts, idrs, vks):
    """Path (a) with the identifier pass on the GPU and on the host, alternating."""
    from plenum_amd.client_authn import GpuAuthNr
    auth = {}
    for name, env in (("gpu_idents", "1"), ("host_idents", "0")):
        os.environ["EDV_WIRE_IDENTS"] = env  # read when the authenticator is made
        a = auth[name] = GpuAuthNr(engine=eng)
        for idr, vk in zip(idrs, vks):
            a.addIdr(idr, vk)
        a.keys_settle()
    os.environ.pop("EDV_WIRE_IDENTS")
    assert auth["gpu_idents"]._g.wire_idents_gpu and not auth["host_idents"]._g.wire_idents_gpu
    for _ in range(2):
        for a in auth.values():
            a.authenticate_wire_batch(texts)
    phases = ("gather", "scan", "keys", "verify", "results")
    times = {k: [] for k in auth}
    breakdown = {k: [] for k in auth}
    for _ in range(args.batches):
        res = {}
        for name, a in auth.items():
            t0 = time.perf_counter()
            res[name] = a.authenticate_wire_batch(texts)
            times[name].append(time.perf_counter() - t0)
            breakdown[name].append(dict(a._g.last_wire_breakdown))
        assert res["gpu_idents"] == res["host_idents"], "results differ between the identifier passes"
        assert all(r.__class__ is str for r in res["gpu_idents"]), "a request of the all-valid batch failed"
        del res
    assert all(a.stats["wire_host_items"] == 0 for a in auth.values()), "the wire scan left items to the host"
    out = {"n": args.n, "signers": args.signers, "batches": args.batches}
    for name in auth:
        ts = [t * 1e3 for t in times[name]]
        out[name] = {"batch_ms": {"p50": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                                  "max": round(max(ts), 3)}}
        for k in phases:
            v = [b[k] for b in breakdown[name]]
            out[name][k + "_ms"] = {"p50": round(statistics.median(v), 3), "min": round(min(v), 3),
                                    "max": round(max(v), 3)}
    return out


def _spread(ts):
    return {"p50": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def digests_probe(eng, args, texts, idrs, vks):
    """Path (a) without digests, with them, and with them the way a caller gets them today."""
    import numpy as np
    from plenum_amd.client_authn import GpuAuthNr
    from plenum_amd.request_digest import request_digests
    a = GpuAuthNr(engine=eng)
    for idr, vk in zip(idrs, vks):
        a.addIdr(idr, vk)
    a.keys_settle()

    def today():
        res = a.authenticate_wire_batch(texts)
        hexes = request_digests([json.loads(t) for t, r in zip(texts, res) if r.__class__ is str], eng)
        return res, hexes

    legs = {"plain": lambda: a.authenticate_wire_batch(texts),
            "digests": lambda: a.authenticate_wire_batch(texts, digests=True),
            "today": today}
    for f in legs.values():  # warm-up: buffers grown, kernels loaded
        f()
    print("warm", flush=True)
    times = {k: [] for k in legs}
    for b in range(args.batches):
        res = {}
        for name, f in legs.items():
            t0 = time.perf_counter()
            res[name] = f()
            times[name].append((time.perf_counter() - t0) * 1e3)
        results, digest, have = res["digests"]
        assert results == res["plain"] == res["today"][0], "verdicts differ between the legs"
        assert have.all() and all(r.__class__ is str for r in results), "a request of the all-valid batch failed"
        want = np.frombuffer(bytes.fromhex("".join(res["today"][1])), np.uint8).reshape(-1, 32)
        assert (digest == want).all(), "digests differ between the GPU's and request_digests"
        del res, results, digest, have, want
        print("batch %d: %s" % (b, {k: round(v[-1], 1) for k, v in times.items()}), flush=True)
    st = a.stats
    assert st["wire_host_items"] == 0 and st["wire_digest_host"] == 0, "items were left to the host"
    out = {"n": args.n, "signers": args.signers, "batches": args.batches,
           "mean_text_bytes": sum(map(len, texts)) / args.n, "wire_digest_gpu": st["wire_digest_gpu"]}
    for name, ts in times.items():
        out[name + "_ms"] = _spread(ts)
    for name in ("digests", "today"):
        out[name + "_added_ms"] = _spread([t - p for t, p in zip(times[name], times["plain"])])
    return out


def node_probe(eng, args, texts, dicts, idrs, vks):
    """Paths (a), (b), (c) over a 4-node and a 25-node pool's drain of about args.n requests."""
    from plenum_amd import nodeloop
    from plenum_amd.batching import requests_in_drain
    from plenum_amd.client_authn import GpuAuthNr
    a, a_split = GpuAuthNr(engine=eng), GpuAuthNr(engine=eng)
    a._g.wire_split_gpu, a_split._g.wire_split_gpu = False, True
    for x in (a, a_split):
        for idr, vk in zip(idrs, vks):
            x.addIdr(idr, vk)
        x.keys_settle()
    phases = ("gather", "scan", "keys", "verify", "results")
    out = {"n": args.n, "signers": args.signers, "batches": args.batches, "members": args.members, "pools": {}}
    for pool in (4, 25):
        reqs = min(len(dicts), max(1, args.n // (pool - 1)))
        entries, bare = [], []
        for g0 in range(0, reqs, args.members):
            group = range(g0, min(reqs, g0 + args.members))
            _, node = nodeloop.drain_texts([dicts[i] for i in group], n_nodes=pool)
            entries += [t.encode() for t, _ in node]
            bare += [texts[i] for i in group] * (pool - 1)
        paths = {
            "node_wire": lambda: a.authenticate_node_wire_batch(entries),
            "node_wire_split": lambda: a_split.authenticate_node_wire_batch(entries),
            "loads_dicts": lambda: a.authenticate_batch(requests_in_drain(entries)),
            "bare_wire": lambda: a.authenticate_wire_batch(bare),
        }
        for f in paths.values():  # warm-up: buffers grown, kernels loaded
            f()
        host0 = a.stats["wire_host_items"], a_split.stats["wire_host_items"]
        times = {k: [] for k in paths}
        breakdown = {"node_wire": [], "node_wire_split": [], "bare_wire": []}
        for _ in range(args.batches):
            res = {}
            for name, f in paths.items():
                t0 = time.perf_counter()
                res[name] = f()
                times[name].append((time.perf_counter() - t0) * 1e3)
                if name in breakdown:
                    breakdown[name].append(dict((a_split if name == "node_wire_split" else a)._g.last_wire_breakdown))
            assert res["node_wire"] == res["node_wire_split"], "results differ between the host and the GPU split"
            flat = [r for per in res["node_wire"] for r in per]  # (per entry: flattened outside the timing)
            assert flat == res["loads_dicts"] == res["bare_wire"], "results differ between the paths"
            assert len(flat) == len(bare) and all(r.__class__ is str for r in flat)
            del flat
            del res
        assert (a.stats["wire_host_items"], a_split.stats["wire_host_items"]) == host0, \
            "the GPU left messages to the host"
        row = {"entries": len(entries), "requests": len(bare), "entry_bytes": sum(map(len, entries)),
               "bare_bytes": sum(map(len, bare))}
        for name, ts in times.items():
            row[name] = {"batch_ms": _spread(ts)}
            for k in phases if name in breakdown else ():
                row[name][k + "_ms"] = _spread([b[k] for b in breakdown[name]])
        p50 = {k: row[k]["batch_ms"]["p50"] for k in paths}
        row["a_over_b"] = round(p50["node_wire"] / p50["loads_dicts"], 4)
        row["a_minus_c_ms"] = round(p50["node_wire"] - p50["bare_wire"], 3)
        row["split_minus_a_ms"] = round(p50["node_wire_split"] - p50["node_wire"], 3)
        out["pools"][str(pool)] = row
        print("pool %d: %s" % (pool, json.dumps(row)), flush=True)
        del entries, bare
    return out


def mixed_probe(eng, args, texts, dicts, idrs, vks):
    """Paths (p), (l), (o) over a 4-node and a 25-node pool's mixed drain, then (l), (o) over the bare texts."""
    from plenum_amd import nodeloop
    from plenum_amd.client_authn import GpuAuthNr
    auth = {}
    for name, (use_list, once) in (("parent", (False, False)), ("list", (True, False)), ("once", (True, True))):
        a = auth[name] = GpuAuthNr(engine=eng)
        a._g.wire_split_gpu, a._g.wire_list, a._g.wire_once = False, use_list, once
        for idr, vk in zip(idrs, vks):
            a.addIdr(idr, vk)
        a.keys_settle()
    phases = ("gather", "scan", "keys", "verify", "results")

    def run(paths, check):
        for f in paths.values():  # warm-up: buffers grown, kernels loaded
            f()
        times = {k: [] for k in paths}
        breakdown = {k: [] for k in paths}
        for _ in range(args.batches):
            res = {}
            for name, f in paths.items():
                t0 = time.perf_counter()
                res[name] = f()
                times[name].append((time.perf_counter() - t0) * 1e3)
                breakdown[name].append(dict(auth[name]._g.last_wire_breakdown))
            first = next(iter(res.values()))
            assert all(r == first for r in res.values()), "results differ between the paths"
            check(first)
            del res, first
        row = {}
        for name, ts in times.items():
            row[name] = {"batch_ms": _spread(ts)}
            for k in phases:
                row[name][k + "_ms"] = _spread([b[k] for b in breakdown[name]])
        return row

    out = {"n": args.n, "signers": args.signers, "batches": args.batches, "members": args.members, "pools": {}}
    for pool in (4, 25):
        reqs = min(len(dicts), max(1, args.n // (pool - 1)))
        entries, n_req = [], 0
        for g0 in range(0, reqs, args.members):
            group = range(g0, min(reqs, g0 + args.members))
            _, node = nodeloop.drain_texts([dicts[i] for i in group], n_nodes=pool)
            for k, (t, _) in enumerate(node):
                entries.append(t.encode())
                entries.append(nodeloop.three_phase_text("PREPARE", pp_seq_no=g0 // args.members + 1).encode())
                entries.append(nodeloop.three_phase_text("COMMIT", pp_seq_no=g0 // args.members + 1).encode())
            n_req += len(group) * (pool - 1)
        stats0 = {k: dict(a.stats) for k, a in auth.items()}

        def check(res, n_req=n_req):
            flat = [r for per in res for r in per]
            assert len(flat) == n_req and all(r.__class__ is str for r in flat)

        row = run({k: (lambda a=a: a.authenticate_node_wire_batch(entries)) for k, a in auth.items()}, check)
        row.update(entries=len(entries), requests=n_req, distinct_requests=reqs, entry_bytes=sum(map(len, entries)))
        calls = args.batches + 1
        for k, a in auth.items():
            assert a.stats["wire_host_items"] == stats0[k]["wire_host_items"], "the GPU left messages to the host"
            row[k]["list_batches"] = (a.stats["wire_list_batches"] - stats0[k]["wire_list_batches"]) // calls
            row[k]["verified_lanes"] = (a.stats["wire_distinct_items"] - stats0[k]["wire_distinct_items"]) // calls
        out["pools"][str(pool)] = row
        print("pool %d: %s" % (pool, json.dumps(row)), flush=True)
        del entries
    bare = {k: (lambda a=auth[k]: a.authenticate_wire_batch(texts)) for k in ("list", "once")}

    def check_bare(res):
        assert len(res) == len(texts) and all(r.__class__ is str for r in res)

    out["bare"] = run(bare, check_bare)
    out["bare"]["requests"] = len(texts)
    print("bare: %s" % json.dumps(out["bare"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--alias-len", type=int, default=43)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-corpus", default=None)
    ap.add_argument("--write-node-corpus", default=None)
    ap.add_argument("--idents-ab", action="store_true")
    ap.add_argument("--digests", action="store_true")
    ap.add_argument("--node", action="store_true")
    ap.add_argument("--mixed", action="store_true", help="--node: PREPARE and COMMIT entries in the drain; list / once A/B")
    ap.add_argument("--members", type=int, default=70, help="--node: PROPAGATEs per BATCH")
    args = ap.parse_args()
    if args.write_corpus:
        return write_corpus(args.write_corpus)
    if args.write_node_corpus:
        return write_node_corpus(args.write_node_corpus)
    from plenum_amd import EdVerifyEngine
    from plenum_amd.client_authn import GpuAuthNr
    eng = EdVerifyEngine(0)
    t0 = time.perf_counter()
    texts, dicts, idrs, vks = build(eng, args.n // 3 if args.node else args.n, args.signers, args.alias_len)
    print("built %d requests, %.0f B mean text, in %.1f s" % (
        args.n, sum(len(t) for t in texts[:1000]) / min(args.n, 1000), time.perf_counter() - t0), flush=True)
    if args.idents_ab or args.node or args.digests:
        line = json.dumps(mixed_probe(eng, args, texts, dicts, idrs, vks) if args.node and args.mixed
                          else node_probe(eng, args, texts, dicts, idrs, vks) if args.node
                          else digests_probe(eng, args, texts, idrs, vks) if args.digests
                          else idents_ab(eng, args, texts, idrs, vks))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        eng.close()
        return
    a = GpuAuthNr(engine=eng)
    for idr, vk in zip(idrs, vks):
        a.addIdr(idr, vk)
    a.keys_settle()
    paths = {
        "wire": lambda: a.authenticate_wire_batch(texts),
        "dicts": lambda: a.authenticate_batch(dicts),
        "loads_dicts": lambda: a.authenticate_batch([json.loads(t) for t in texts]),
    }
    for _ in range(2):  # warm-up: buffers grown, kernels loaded
        for f in paths.values():
            f()
    host0 = a.stats["wire_host_items"]
    times = {k: [] for k in paths}
    breakdown = []
    for _ in range(args.batches):
        res = {}
        for name, f in paths.items():
            t0 = time.perf_counter()
            res[name] = f()
            times[name].append(time.perf_counter() - t0)
            if name == "wire":
                breakdown.append(dict(a._g.last_wire_breakdown))
        assert res["wire"] == res["dicts"] == res["loads_dicts"], "verdicts differ between the paths"
        assert all(r.__class__ is str for r in res["wire"]), "a request of the all-valid batch failed"
        del res
    assert a.stats["wire_host_items"] == host0, "the wire scan left items to the host"
    out = {"n": args.n, "signers": args.signers, "batches": args.batches,
           "mean_text_bytes": sum(map(len, texts)) / args.n}
    for name, ts in times.items():
        p50 = statistics.median(ts)
        out[name] = {"p50_ms": round(p50 * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
                     "max_ms": round(max(ts) * 1e3, 3),
                     "M_requests_per_s": round(args.n / p50 / 1e6, 3)}
    out["wire_breakdown_p50_ms"] = {k: round(statistics.median(b[k] for b in breakdown), 3)
                                    for k in ("gather", "scan", "keys", "verify", "results")}
    out["wire_breakdown_note"] = ("gather = texts into pinned memory; scan = PCIe + edv_wire_scan_kernel + status "
                                  "read-back; "
                                  "keys = distinct identifiers, getVerkey, key ids; verify = edv_wire_verify; "
                                  "results = the result list")
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
