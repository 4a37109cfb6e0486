#!/usr/bin/env python3
"""ElGamal decryption on the GPU (zk_elgamal_table_create / zk_elgamal_decrypt) against the reference's walk: ONE JSON line.

  table_create_ms       cold zk_elgamal_table_create, baby_bits = 20 (the first in the process: code objects load in it too)
  n1_ref                warm n = 1 at the reference's limit 10^6: median / min of 25 calls
  n1_u32                n = 1 at 2^32 (median of 9)
  n1024_ref, n1024_u32  n = 1024 at both limits (median of 5)
  each with wall_ms (the whole entry, host clock around a call that ends in a device synchronise), device_ms (HIP events around
  the search kernel, zk_profile_*) and host_ms = wall - device (decoding, dk * right, copies, launch)
  cpu_baseline          tools/ubench/elgamal_walk.cpp: the reference's loop (elgamal.rs:92-107) on one core for v = 999 999
Usage: python tools/decrypt_probe.py [out.json]
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_baseline(value=999999):
    src = os.path.join(ROOT, "tools", "ubench", "elgamal_walk.cpp")
    rocm_cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = rocm_cxx if os.path.exists(rocm_cxx) else "c++"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "elgamal_walk")
        subprocess.check_call([cxx, "-O2", "-std=c++17", src, "-o", exe])
        runs = [json.loads(subprocess.check_output([exe, str(value)]).decode()) for _ in range(3)]
    best = min(runs, key=lambda r: r["ms"])
    return dict(best, runs_ms=[r["ms"] for r in runs])


def main():
    import numpy as np
    import zero_chain_amd as zk
    lib = zk.load_library()
    rng = np.random.default_rng(7)
    dk = 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcd
    (enc_key,) = zk.jubjub_base_mul([dk], lib=lib)

    def ciphertexts(vals):
        rnd = [int.from_bytes(rng.bytes(31), "little") for _ in vals]
        return zk.elgamal_encrypt(vals, rnd, [enc_key] * len(vals), lib=lib)

    def timed(t, left, right, limit, reps, want):
        walls, devs = [], []
        for _ in range(reps):
            with zk.KernelTimer(lib) as kt:
                t0 = time.perf_counter()
                got = t.decrypt(left, right, dk, limit=limit)
                walls.append((time.perf_counter() - t0) * 1e3)
                devs.append(kt.get("elgamal_dlog")[1])
            assert got == want, "wrong result"
        wall, dev = statistics.median(walls), statistics.median(devs)
        return {"n": len(left), "limit": limit, "reps": reps, "wall_ms": round(wall, 4), "wall_min_ms": round(min(walls), 4),
                "device_ms": round(dev, 4), "host_ms": round(wall - dev, 4)}

    out = {"probe": "decrypt", "baby_bits": 20}
    with zk.KernelTimer(lib) as kt:
        t0 = time.perf_counter()
        table = zk.ElGamalTable(20, lib=lib)
        out["table_create_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["table_create_device_ms"] = round(kt.get("elgamal_table")[1], 3)
    with zk.ElGamalTable(20, lib=lib):   # a second, warm creation
        pass
    t0 = time.perf_counter()
    again = zk.ElGamalTable(20, lib=lib)
    out["table_create_warm_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    again.close()
    out["table_device_bytes"] = (1 << 20) * 64 + (1 << 21) * 8
    try:
        l1, r1 = ciphertexts([999999])
        timed(table, l1, r1, zk.ELGAMAL_DECRYPT_LIMIT, 3, [999999])   # warm-up of both paths
        lu, ru = ciphertexts([4000000000])
        timed(table, lu, ru, 1 << 32, 2, [4000000000])
        out["n1_ref"] = timed(table, l1, r1, zk.ELGAMAL_DECRYPT_LIMIT, 25, [999999])
        out["n1_u32"] = timed(table, lu, ru, 1 << 32, 9, [4000000000])
        vals = [int(v) for v in rng.integers(0, zk.ELGAMAL_DECRYPT_LIMIT, 1024)]
        lb, rb = ciphertexts(vals)
        out["n1024_ref"] = timed(table, lb, rb, zk.ELGAMAL_DECRYPT_LIMIT, 5, vals)
        vals32 = [int(v) for v in rng.integers(0, 1 << 32, 1024, dtype=np.uint64)]
        lb, rb = ciphertexts(vals32)
        out["n1024_u32"] = timed(table, lb, rb, 1 << 32, 5, vals32)
    finally:
        table.close()
    out["cpu_baseline"] = cpu_baseline()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
