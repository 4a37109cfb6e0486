#!/usr/bin/env python3
"""What ElGamal encryption of groups of keys costs (zk_elgamal_encrypt_dev, csrc/elgamal_encrypt.h) beside zk_elgamal_encrypt on
the same items in the same process: ONE JSON line.

  n groups of k keys for k in 1, 3, 12 and n in 1, 4, 16, 64, 256, 1024, 4096, every key distinct (n k decode lanes: the worst
  case for the device form), the values non-negative so that zk_elgamal_encrypt can encrypt the same items (k = 3: amount, amount,
  fee; k = 12: two amounts and ten zeros), on 16 host threads.  Per (k, n), wall ms (host clock around the entry, which ends in a
  device synchronise; one warm repetition discarded, median of five with min and max, the columns taken in turn inside every
  repetition):
    host      ZKAMD_ENCRYPT_HOST_MAX huge: the host threads
    device    ZKAMD_ENCRYPT_HOST_MAX=0: k_derive_points, k_derive_combine (csrc/derive_stage.h)
    default   the variable unset
    old       ONE call of zk_elgamal_encrypt over the n k items, the randomness of a group repeated for each of its keys
  and the totals of the device form's stages (HIP events, zk_profile_*) in runs of their own: encrypt_upload, encrypt_points,
  encrypt_combine, encrypt_download.  "crossover": the largest probed n k at which the host form's median is below the device
  form's, 0 if there is none - the default of ZKAMD_ENCRYPT_HOST_MAX.
Usage: python tools/encrypt_probe.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 3, 12)
SIZES = (1, 4, 16, 64, 256, 1024, 4096)
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
VAR = "ZKAMD_ENCRYPT_HOST_MAX"
STAGES = ("encrypt_upload", "encrypt_points", "encrypt_combine", "encrypt_download")
FS_MOD = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
FORMS = (("host", str(1 << 40)), ("device", "0"), ("default", None))


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


def group_values(rng, k):
    amount = 1 + rng.below(1 << 20)
    if k == 3:
        return [amount, amount, 1 + rng.below(100)]
    if k == 12:
        s = rng.below(12)
        t = (s + 1 + rng.below(11)) % 12
        return [amount if j in (s, t) else 0 for j in range(12)]
    return [amount] * k


def main():
    import numpy as np
    import zero_chain_amd as zk
    from oracle import synth
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    rng = synth.SplitMix64(33)
    fs = lambda: rng.field(FS_MOD)
    top = max(SIZES) * max(KS)
    all_keys = np.frombuffer(b"".join(zk.jubjub_base_mul([fs() for _ in range(top)], lib=lib)), dtype=np.uint8).copy()
    all_rnd = zk.scalars_to_bytes([fs() for _ in range(max(SIZES))])
    result = {"tool": "tools/encrypt_probe.py", "host_threads": HOST_THREADS, "rows": {}}
    crossover = 0
    for k in KS:
        for n in SIZES:
            nk = n * k
            vals = [v for _ in range(n) for v in group_values(rng, k)]
            v64, v32 = np.asarray(vals, dtype=np.int64), np.asarray(vals, dtype=np.uint32)
            keys, rnd = all_keys[:32 * nk].copy(), all_rnd[:32 * n].copy()
            rnd_each = np.repeat(rnd.reshape(n, 32), k, axis=0).reshape(-1).copy()
            left, right, st = np.zeros(32 * nk, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8), np.zeros(nk, dtype=np.uint8)
            old_left, old_right = np.zeros(32 * nk, dtype=np.uint8), np.zeros(32 * nk, dtype=np.uint8)
            call = lambda: lib.check(lib.zk_elgamal_encrypt_dev(n, k, ptr(v64), ptr(rnd), ptr(keys), 0, ptr(left), ptr(right), ptr(st)))
            old = lambda: lib.check(lib.zk_elgamal_encrypt(ptr(v32), ptr(rnd_each), ptr(keys), nk, ptr(old_left), ptr(old_right)))
            row = timed([(name, with_form(value, call)) for name, value in FORMS] + [("old", old)])
            row["same_bytes_as_old"] = bool((left == old_left).all() and (right.reshape(n, 32) == old_right.reshape(n, k, 32)[:, 0]).all() and not st.any())
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
            if row["host"]["median_ms"] < row["device"]["median_ms"]:
                crossover = max(crossover, nk)
            result["rows"]["k=%d n=%d" % (k, n)] = row
            print("k", k, "n", n, json.dumps(row), file=sys.stderr, flush=True)
    result["crossover"] = crossover
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
