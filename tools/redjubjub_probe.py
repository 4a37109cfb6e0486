#!/usr/bin/env python3
"""What checking the signatures of a block costs (zk_redjubjub_verify_batch), in its two forms and as the library chooses between
them, and what signing costs (zk_redjubjub_sign): ONE JSON line.

  per n in 1, 64, 256, 1024, 4096 signatures, wall ms (host clock around the entry, which ends in a device synchronise; two warm
  repetitions discarded, median of seven with min and max, the three forms taken in turn inside every repetition):
    host      ZKAMD_REDJUBJUB_HOST_MAX huge: decode and the joint multiplication on the host threads
    device    ZKAMD_REDJUBJUB_HOST_MAX=0: the two kernels, the messages hashed on the host beside the first
    default   the variable unset
  sign: zk_redjubjub_sign at n = 1 and 1024, the same way.
The signatures: 64 distinct accepted ones (random keys, messages of 0 .. 300 bytes), repeated up to n.
Usage: python tools/redjubjub_probe.py [out.json]
"""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 64
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
ENV = "ZKAMD_REDJUBJUB_HOST_MAX"


def main():
    import numpy as np
    import zero_chain_amd as zk
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = random.Random(9)
    sks = [rng.randrange(1, FS_MODULUS) for _ in range(DISTINCT)]
    base_msgs = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 301))) for _ in range(DISTINCT)]
    base_ts = [bytes(rng.randrange(256) for _ in range(80)) for _ in range(DISTINCT)]
    base_vks = zk.jubjub_base_mul(sks, lib=lib)
    base_sigs = zk.redjubjub_sign(sks, base_ts, base_msgs, lib=lib)
    assert zk.redjubjub_verify(base_vks, base_sigs, base_msgs, lib=lib) == ([True] * DISTINCT, [0] * DISTINCT)

    def block(n, parts):
        return np.frombuffer(b"".join(parts[i % DISTINCT] for i in range(n)) or b"\0", dtype=np.uint8).copy()

    def offsets(n):
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(base_msgs[i % DISTINCT]) for i in range(n)], dtype=np.uint64)
        return offs

    def timed(runs, check, warm=2, reps=7):
        walls = {name: [] for name, _ in runs}
        for rep in range(warm + reps):
            for name, fn in runs:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                check()
                if rep >= warm:
                    walls[name].append(dt)
        return {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}
                for name, w in walls.items()}

    out = {"probe": "redjubjub", "host_threads": HOST_THREADS, "distinct": DISTINCT, "verify": {}, "sign": {}}
    for n in (1, 64, 256, 1024, 4096):
        vks, sigs, msgs, offs = block(n, base_vks), block(n, base_sigs), block(n, base_msgs), offsets(n)
        ok = np.zeros(n, dtype=np.uint8)

        def entry(host_max):
            def run():
                if host_max is None:
                    os.environ.pop(ENV, None)
                else:
                    os.environ[ENV] = host_max
                lib.check(lib.zk_redjubjub_verify_batch(n, ptr(vks), ptr(sigs), ptr(msgs), ptr(offs), 0, ptr(ok), None))
            return run

        def check():
            assert ok.all(), "a signature of the block was not accepted"
            ok[:] = 0
        out["verify"][str(n)] = timed([("host", entry("1000000000")), ("device", entry("0")), ("default", entry(None))], check)
    os.environ.pop(ENV, None)
    for n in (1, 1024):
        keys, ts, msgs, offs = block(n, [k.to_bytes(32, "little") for k in sks]), block(n, base_ts), block(n, base_msgs), offsets(n)
        sig_out = np.zeros(64 * n, dtype=np.uint8)

        def run():
            lib.check(lib.zk_redjubjub_sign(n, ptr(keys), ptr(ts), ptr(msgs), ptr(offs), ptr(sig_out)))

        def check():
            assert sig_out[:64].tobytes() == base_sigs[0]
            sig_out[:] = 0
        out["sign"][str(n)] = timed([("sign", run)], check)["sign"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
