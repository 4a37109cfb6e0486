#!/usr/bin/env python3
"""zk_verify_batch at several batch sizes under the forms of verify_chunk, and zk_verify_batch_rlc (from 8 proofs), on the GPU
box: wall time per call, best of 6.
   python tools/verify_n_probe.py [--forms rows,rlc] [--json PATH] [n ...]
   forms: rows (default), pairing (ZKAMD_COOP_PAIRING=0), lanes (ZKAMD_COOP_VERIFY=0), rlc (the combined check)
   --json PATH: the six times of every (n, form) as one JSON object, for records under profiles/"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.cuda.set_device(0)
import zero_chain_amd as zk
import helpers
import importlib.util
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py")); bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
from oracle import bls12_381 as bls, synth
args, only, json_path = sys.argv[1:], None, None
while args and args[0].startswith("--"):
    if args[0] == "--forms": only = args[1].split(",")
    elif args[0] == "--json": json_path = args[1]
    else: sys.exit(__doc__)
    args = args[2:]
lib = zk.load_library()
mats = zk.ConstraintMatrices.transfer_circuit(lib=lib)
params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=lib)
pvk = zk.prepare_verifying_key(params)
M = 16
sts = zk.transfer_statements(bench.make_statements_native(zk, lib, 0, M))
rng = synth.SplitMix64(5)
rs = [(rng.field(bls.R_MOD), rng.field(bls.R_MOD)) for _ in range(M)]
raw = np.frombuffer(b"".join(p.write() for p in zk.transfer_prove_batch(mats, params, sts, rs)), dtype=np.uint8).copy().reshape(M, 192)
w = zk.transfer_witness(sts, lib=lib).reshape(M, -1)
pub = np.ascontiguousarray(w[:, 32:zk.TRANSFER_N_INPUTS * 32])
sizes = [int(a) for a in args] or [1, 16, 64, 256, 1024, 2048]
forms = (("rows", {}, False), ("pairing", {"ZKAMD_COOP_PAIRING": "0"}, False), ("lanes", {"ZKAMD_COOP_VERIFY": "0"}, False), ("rlc", {}, True))
record = {}
for n in sizes:
    idx = np.arange(n) % M
    pr, pi = np.ascontiguousarray(raw[idx]).reshape(-1), np.ascontiguousarray(pub[idx]).reshape(-1)
    bad = pr.copy(); bad[192 * (n - 1) + 100] ^= 1      # the last proof's B is another point (or none)
    line = []
    for name, env, rlc in forms:
        if (only and name not in only) or (rlc and n < 8): continue
        for k in ("ZKAMD_COOP_PAIRING", "ZKAMD_COOP_VERIFY"): os.environ.pop(k, None)
        os.environ.update(env)
        assert all(zk.verify_proofs(pvk, pr, pi, rlc=rlc)), (n, name)
        got = zk.verify_proofs(pvk, bad, pi, rlc=rlc)
        assert all(got[:-1]) and not got[-1], (n, name)
        ts = []
        for _ in range(6):
            t0 = time.perf_counter(); zk.verify_proofs(pvk, pr, pi, rlc=rlc); ts.append((time.perf_counter() - t0) * 1e3)
        line.append("%s %.2f" % (name, min(ts)))
        record["%s n=%d" % (name, n)] = [round(t, 3) for t in ts]
    print("n = %5d: %s ms" % (n, " | ".join(line)), flush=True)
print("memory:", json.dumps(zk.memory_stats(lib)), flush=True)   # (what the key and the workspaces hold: the same for the same arguments)
if json_path:
    with open(json_path, "w") as f: json.dump(record, f)
