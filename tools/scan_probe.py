#!/usr/bin/env python3
"""What reading a block with one decryption key costs (zk_confidential_scan / zk_anonymous_scan), with the point work in its two
forms and as the library chooses between them, beside the same values through zk_elgamal_decrypt: ONE JSON line.

  confidential: per n in 1, 16, 64, 128, 256, 512, 1024, 4096 extrinsics that all match as recipient (one row each), limit 10^6,
  wall ms (host clock around the entry, which ends in a device synchronise; two warm repetitions discarded, median of seven with
  min and max, the four taken in turn inside every repetition):
    host      ZKAMD_SCAN_HOST_MAX huge: decoding and dk * right on the host threads, one upload, the search
    device    ZKAMD_SCAN_HOST_MAX=0: k_scan_points + k_scan_combine, then the search on the resident rows
    default   the variable unset
    decrypt   zk_elgamal_decrypt on the same (left_amount_recipient, right_randomness) pairs: how the same numbers were had
              before the scan existed
  and the device time of the stage's two kernels (HIP events, zk_profile_*) in a run of their own per n.
  anonymous: 1024 extrinsics with the key once in each (sender, recipient and decoy in turn), limits 10^6 and 2^32, the three forms.
The extrinsics: 64 distinct ones (random amounts below 10^6, zeroed proofs), repeated up to n.
Usage: python tools/scan_probe.py [out.json]
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
ENV = "ZKAMD_SCAN_HOST_MAX"
LIMIT = 1000000


def main():
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = random.Random(14)
    fs = lambda: rng.randrange(1, FS_MODULUS)
    wallet = fs()
    strangers = zk.jubjub_base_mul([fs() for _ in range(12)], lib=lib)
    (key,) = zk.jubjub_base_mul([wallet], lib=lib)
    kb = np.frombuffer(wallet.to_bytes(32, "little"), dtype=np.uint8).copy()

    amounts = [rng.randrange(LIMIT) for _ in range(DISTINCT)]
    rnd = [fs() for _ in range(DISTINCT)]
    ls, _ = zk.elgamal_encrypt(amounts, rnd, [strangers[0]] * DISTINCT, lib=lib)
    lr, right = zk.elgamal_encrypt(amounts, rnd, [key] * DISTINCT, lib=lib)
    lf, _ = zk.elgamal_encrypt([1] * DISTINCT, rnd, [strangers[0]] * DISTINCT, lib=lib)
    conf = (_lib.ConfidentialXt * DISTINCT)()
    for i, x in enumerate(conf):
        x.enc_key_sender[:], x.enc_key_recipient[:] = strangers[0], key
        x.left_amount_sender[:], x.left_amount_recipient[:], x.left_fee[:], x.right_randomness[:] = ls[i], lr[i], lf[i], right[i]

    signs = [(1, -1, 0)[i % 3] for i in range(DISTINCT)]
    anon = (_lib.AnonymousXt * DISTINCT)()
    for i, x in enumerate(anon):
        at = i % 12
        keys = [key if k == at else strangers[k] for k in range(12)]
        lefts, rights = zk.elgamal_encrypt([amounts[i] if k == at and signs[i] > 0 else 0 for k in range(12)], [rnd[i]] * 12, keys, lib=lib)
        if signs[i] < 0:
            (la,), (ra,) = zk.elgamal_encrypt([amounts[i]], [0], [key], lib=lib)
            (lefts[at],), _ = zk.elgamal_add([lefts[at]], [rights[at]], [la], [ra], subtract=True, lib=lib)
        for k in range(12):
            x.enc_keys[k][:], x.left_ciphertexts[k][:] = keys[k], lefts[k]
        x.right_ciphertext[:] = rights[0]

    def repeat(base, n):
        arr = (base._type_ * n)()
        for first in range(0, n, DISTINCT):
            count = min(DISTINCT, n - first)
            C.memmove(C.byref(arr, first * C.sizeof(base._type_)), base, count * C.sizeof(base._type_))
        return arr

    def timed(runs, check, warm=2, reps=7):
        walls = {name: [] for name, _ in runs}
        for rep in range(warm + reps):
            for name, fn in runs:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                check(name)
                if rep >= warm:
                    walls[name].append(dt)
        return {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}
                for name, w in walls.items()}

    def with_env(host_max, fn):
        def run():
            if host_max is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = host_max
            fn()
        return run

    out = {"probe": "scan", "host_threads": HOST_THREADS, "distinct": DISTINCT, "limit": LIMIT, "confidential": {}, "anonymous": {}}
    table = zk.ElGamalTable(lib=lib)
    try:
        for n in (1, 16, 64, 128, 256, 512, 1024, 4096):
            xts = repeat(conf, n)
            res = (_lib.ConfidentialScanResult * n)()
            left = np.frombuffer(b"".join(lr[i % DISTINCT] for i in range(n)), dtype=np.uint8).copy()
            rgt = np.frombuffer(b"".join(right[i % DISTINCT] for i in range(n)), dtype=np.uint8).copy()
            vals, found = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
            want = [amounts[i % DISTINCT] for i in range(n)]

            def scan():
                lib.check(lib.zk_confidential_scan(table._h, n, xts, ptr(kb), LIMIT, res))

            def decrypt():
                lib.check(lib.zk_elgamal_decrypt(table._h, n, ptr(left), ptr(rgt), ptr(kb), 0, LIMIT, ptr(vals), ptr(found)))

            def check(name):
                if name == "decrypt":
                    assert found.all() and vals.tolist() == want, "zk_elgamal_decrypt: a wrong value"
                    vals[:] = 0
                    found[:] = 0
                else:
                    assert all(r.role == 2 and r.found == 4 and r.refusal == 0 for r in res) and [r.amount_received for r in res] == want, name
                    C.memset(res, 0, C.sizeof(res))
            row = timed([("host", with_env("1000000000", scan)), ("device", with_env("0", scan)), ("default", with_env(None, scan)),
                         ("decrypt", decrypt)], check)
            os.environ[ENV] = "0"
            with zk.KernelTimer(lib) as kt:
                scan()
                row["device_kernels_ms"] = {k: round(kt.get(k)[1], 4) for k in ("scan_points", "scan_combine", "elgamal_dlog")}
            out["confidential"][str(n)] = row
        n = 1024
        xts = repeat(anon, n)
        res = (_lib.AnonymousScanResult * n)()
        want = [signs[i % DISTINCT] * amounts[i % DISTINCT] for i in range(n)]
        for limit in (LIMIT, 1 << 32):
            def scan():
                lib.check(lib.zk_anonymous_scan(table._h, n, xts, ptr(kb), limit, res))

            def check(name):
                assert all(r.found == 1 and r.refusal == 0 for r in res) and [r.delta for r in res] == want, name
                C.memset(res, 0, C.sizeof(res))
            row = timed([("host", with_env("1000000000", scan)), ("device", with_env("0", scan)), ("default", with_env(None, scan))], check)
            os.environ[ENV] = "0"
            with zk.KernelTimer(lib) as kt:
                scan()
                row["device_kernels_ms"] = {k: round(kt.get(k)[1], 4) for k in ("scan_points", "scan_combine", "elgamal_dlog")}
            out["anonymous"]["%d@%d" % (n, limit)] = row
    finally:
        os.environ.pop(ENV, None)
        table.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
