#!/usr/bin/env python3
"""What the request -> statement derivation of the anonymous transfer costs (zk_anonymous_derive_dev, csrc/anon_derive.h), and
what zk_anonymous_gen_proof_batch costs with it: ONE JSON line.

  derive: n requests that share nothing but g_epoch (35 n + 1 distinct encodings), with the 104 public inputs, for n in 1, 8, 64,
  256, 1024, 4096 on 16 host threads.  Per n, wall ms (host clock around the entry, which ends in a device synchronise; one warm
  repetition discarded, median of five with min and max, the columns taken in turn inside every repetition):
    host      ZKAMD_ANON_DERIVE_HOST_MAX huge: anonymous_derive_one on the host threads
    device    ZKAMD_ANON_DERIVE_HOST_MAX=0: the host part, k_derive_points, k_derive_combine (csrc/derive_stage.h)
    default   the variable unset
  and the totals of the device form's stages (HIP events, zk_profile_*) in runs of their own: anon_derive_host (the checks, [sk]G,
  the hash, the Fs products: events on an idle stream, so host time), anon_derive_upload, anon_derive_points, anon_derive_combine,
  anon_derive_download.
  gen_proof: zk_anonymous_gen_proof_batch of 512 and 1024 consistent requests, the same columns, in a process of its own; with
  --parent-lib PATH (a libzkamd.so built from the parent commit) also that library's, in another process right after it.
Usage: python tools/anon_derive_probe.py [out.json] [--parent-lib PATH]
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1, 8, 64, 256, 1024, 4096)
GEN_PROOF_SIZES = (512, 1024)
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
VAR = "ZKAMD_ANON_DERIVE_HOST_MAX"
STAGES = ("anon_derive_host", "anon_derive_upload", "anon_derive_points", "anon_derive_combine", "anon_derive_download")
FS_MOD = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7


def make_requests(zk, lib, n, seed=7):
    """n consistent requests: the sender's balance encrypts `balance` under its own key, everything else is random prime-order points"""
    from oracle import synth
    rng = synth.SplitMix64(seed)
    fs = lambda: rng.field(FS_MOD)
    pts = zk.jubjub_base_mul([fs() for _ in range(35 * n + 1)], lib=lib)
    g_epoch, pts = pts[0], pts[1:]
    items = []
    for i in range(n):
        p = pts[35 * i:35 * i + 35]
        s = rng.below(12)
        t = (s + 1 + rng.below(11)) % 12
        balance = 1000 + rng.below(1 << 20)
        amount = rng.below(1000)
        items.append(dict(amount=amount, remaining_balance=balance - amount, s_index=s, t_index=t, spending_key=fs(), enc_key_recipient=p[0],
                          enc_keys_decoy=p[1:11], enc_balances_left=p[11:23], enc_balances_right=p[23:35], g_epoch=g_epoch, randomness=fs(), alpha=fs()))
    # the sender's own balance under the sender's own key
    os.environ[VAR] = str(1 << 40)
    sts, _ = zk.anonymous_derive(zk.anonymous_requests(items), lib=lib)
    keys = [bytes(st.enc_keys[it["s_index"]]) for st, it in zip(sts, items)]
    left, right = zk.elgamal_encrypt([it["amount"] + it["remaining_balance"] for it in items], [fs() for _ in items], keys, lib=lib)
    for it, l, r in zip(items, left, right):
        it["enc_balances_left"] = it["enc_balances_left"][:it["s_index"]] + [l] + it["enc_balances_left"][it["s_index"] + 1:]
        it["enc_balances_right"] = it["enc_balances_right"][:it["s_index"]] + [r] + it["enc_balances_right"][it["s_index"] + 1:]
    os.environ.pop(VAR, None)
    return items


def timed(runs, warm=1, reps=5):
    walls = {name: [] for name, _ in runs}
    for rep in range(warm + reps):
        for name, fn in runs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                walls[name].append(dt)
    return {name: {"median_ms": round(statistics.median(w), 3), "min_ms": round(min(w), 3), "max_ms": round(max(w), 3)} for name, w in walls.items()}


def with_form(value, fn):
    def run():
        if value is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = value
        try:
            return fn()
        finally:
            os.environ.pop(VAR, None)
    return run


FORMS = (("host", str(1 << 40)), ("device", "0"), ("default", None))


def ParentLib(path):
    """the parent commit's library behind this tree's prototypes, less the entry it does not have"""
    from zero_chain_amd import _lib
    protos = dict(_lib._PROTOS)
    del _lib._PROTOS["zk_anonymous_derive_dev"]
    try:
        return _lib.ZkLib(path)
    finally:
        _lib._PROTOS.clear()
        _lib._PROTOS.update(protos)


def gen_proof_child(path, forms):
    """zk_anonymous_gen_proof_batch through the library at `path`: one JSON line {n: {form: wall ms ..., "sha256": of the extrinsics}}"""
    import hashlib
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    import helpers
    from oracle import bls12_381 as bls
    from oracle import synth
    try:
        lib = _lib.ZkLib(path)
    except AttributeError:
        lib = ParentLib(path)
    lib.zk_set_host_threads(HOST_THREADS)
    items = make_requests(zk, lib, max(GEN_PROOF_SIZES))
    mats = zk.ConstraintMatrices.anonymous_circuit(lib=lib)
    params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=lib)
    pvk = zk.prepare_verifying_key(params)
    rng = synth.SplitMix64(4242)
    values = dict(FORMS)
    rows, last = {}, {}
    for n in GEN_PROOF_SIZES:
        arr = zk.anonymous_requests(items[:n])
        rs = zk.scalars_to_bytes([rng.field(bls.R_MOD) for _ in range(2 * n)])

        def run():
            last["xts"] = zk.anonymous_gen_proofs(params, mats, pvk, arr, rs)
        rows[str(n)] = timed([(f, with_form(values[f], run)) for f in forms])
        rows[str(n)]["sha256"] = hashlib.sha256(repr(last["xts"]).encode()).hexdigest()
    pvk.close()
    params.close()
    mats.close()
    print(json.dumps(rows))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--gen-proof-child":
        return gen_proof_child(sys.argv[2], sys.argv[3].split(","))
    import ctypes as C
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = sys.argv[1:]
    parent_path = None
    if "--parent-lib" in args:
        k = args.index("--parent-lib")
        parent_path = args[k + 1]
        del args[k:k + 2]
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    result = {"tool": "tools/anon_derive_probe.py", "host_threads": HOST_THREADS, "derive": {}, "gen_proof": {}}
    all_items = make_requests(zk, lib, max(SIZES + GEN_PROOF_SIZES))
    for n in SIZES:
        arr = zk.anonymous_requests(all_items[:n])
        st, rsk, inputs = (_lib.AnonymousStatement * n)(), np.zeros(32 * n, dtype=np.uint8), np.zeros(104 * 32 * n, dtype=np.uint8)
        # (the entry itself: the Python wrapper's conversion of 104 n integers is not the library's time)
        call = lambda: lib.check(lib.zk_anonymous_derive_dev(arr, n, 0, st, ptr(rsk), ptr(inputs)))
        row = timed([(name, with_form(value, call)) for name, value in FORMS])
        stages = {s: [] for s in STAGES}
        for rep in range(6):
            with zk.KernelTimer(lib) as t:
                with_form("0", call)()
                got = {s: t.get(s) for s in STAGES}
            if rep:
                for s in STAGES:
                    stages[s].append(got[s][1])
        row["device_stages_ms"] = {s: round(statistics.median(v), 3) for s, v in stages.items()}
        row["launches"] = {s: got[s][0] for s in STAGES}
        result["derive"][str(n)] = row
        print("derive", n, json.dumps(row), file=sys.stderr, flush=True)

    # gen_proof: a process per library, one after the other (the chunk workspaces of two libraries do not fit one device together)
    def child(path, forms):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--gen-proof-child", path, ",".join(forms)], check=True, capture_output=True, text=True)
        sys.stderr.write(out.stderr[-2000:])
        return json.loads(out.stdout.strip().splitlines()[-1])
    rows = child(lib.path, [f for f, _ in FORMS])
    if parent_path:
        parent_rows = child(parent_path, ["default"])
        for n in rows:
            rows[n]["parent"] = parent_rows[n]["default"]
            rows[n]["same_bytes_as_parent"] = rows[n].pop("sha256") == parent_rows[n]["sha256"]
    result["gen_proof"] = rows
    print("gen_proof", json.dumps(rows), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args:
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
