#!/usr/bin/env python3
"""What judging a block of confidential transfers from their BYTES costs (zk_confidential_verify_batch) beside verifying the
same proofs with ready-made inputs (zk_verify_batch): ONE JSON line.

  per n in 1, 64, 1024, 4096 transactions, wall ms (host clock around an entry that ends in a device synchronise; two warm
  repetitions discarded, median of seven, the four forms taken in turn inside every repetition):
    a_inputs_ready   zk_verify_batch, the 22 inputs per proof prepared beforehand: what the library could do before, the floor
    b_host           zk_confidential_verify_batch, IntoXY on the host threads     (ZKAMD_INTO_XY_HOST_MAX huge)
    c_device         the same, IntoXY on the device                               (ZKAMD_INTO_XY_HOST_MAX=0)
    d_default        the same, the variable unset
  into_xy: zk_jubjub_into_xy alone at several point counts, both forms - where they cross is ZKAMD_INTO_XY_HOST_MAX's default.
The transactions: 64 distinct ones (eleven prime-order points each, a proof made from the trapdoor of a synthetic 22-input key,
so that every one verifies), repeated up to n; one g_epoch per transaction (stride 32), balances in the xt.
Usage: python tools/xt_verify_probe.py [out.json]          the measurements
       python tools/xt_verify_probe.py --kernel-only N     N transactions through form (c) a few times: the run to put under
                                                           rocprofv3 --kernel-trace --stats for the kernel's own duration
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT = 64
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
A, B = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321


def main():
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib as zl
    from oracle import bls12_381 as bls
    import helpers
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    r1, asg, P, pk = helpers.small_case(31, 23, 6, 30)
    n_ic = int.from_bytes(pk[864:868], "big")
    pvk = zk.prepare_verifying_key(pk[:868 + 96 * n_ic], lib=lib)
    rng = random.Random(5)
    points = zk.jubjub_base_mul([rng.randrange(1, FS_MODULUS) for _ in range(11 * DISTINCT)], lib=lib)
    coords, st = zk.jubjub_into_xy(points, lib=lib)
    assert not any(st)
    sc, r = P.sc, bls.R_MOD
    g1 = lambda k: bls.g1_compressed(bls.G1.to_affine(bls.G1.mul(bls.G1_GEN, k % r)))
    pa, pb = g1(A), bls.g2_compressed(bls.G2.to_affine(bls.G2.mul(bls.G2_GEN, B)))
    base_xt, base_inputs, base_proofs, base_epochs = (zl.ConfidentialXt * DISTINCT)(), [], [], []
    for i in range(DISTINCT):
        p, xy = points[11 * i:11 * i + 11], [v for c in coords[11 * i:11 * i + 11] for v in c]
        acc = (sc["ic"][0] + sum(x * k for x, k in zip(xy, sc["ic"][1:]))) % r
        proof = pa + pb + g1((A * B - sc["alpha"] * sc["beta"] - sc["gamma"] * acc) * pow(sc["delta"], -1, r))
        x = base_xt[i]
        for f, v in (("proof", proof), ("enc_key_sender", p[0]), ("enc_key_recipient", p[1]), ("left_amount_sender", p[2]),
                     ("left_amount_recipient", p[3]), ("right_randomness", p[4]), ("left_fee", p[5]), ("enc_balance", p[6] + p[7]),
                     ("rvk", p[8]), ("nonce", p[10])):
            getattr(x, f)[:] = v
        base_inputs.append(zk.scalars_to_bytes(xy).tobytes())
        base_proofs.append(proof)
        base_epochs.append(p[9])

    def block(n):
        xts = (zl.ConfidentialXt * n)()
        for i in range(n):
            C.memmove(C.byref(xts[i]), C.byref(base_xt[i % DISTINCT]), C.sizeof(zl.ConfidentialXt))
        cat = lambda items: np.frombuffer(b"".join(items[i % DISTINCT] for i in range(n)), dtype=np.uint8).copy()
        return xts, cat(base_proofs), cat(base_inputs), cat(base_epochs)

    def forms(n):
        xts, proofs, inputs, epochs = block(n)
        ok = np.zeros(n, dtype=np.uint8)

        def a():
            lib.check(lib.zk_verify_batch(pvk._h, n, ptr(proofs), ptr(inputs), 22, ptr(ok)))

        def entry(host_max):
            def run():
                if host_max is None:
                    os.environ.pop("ZKAMD_INTO_XY_HOST_MAX", None)
                else:
                    os.environ["ZKAMD_INTO_XY_HOST_MAX"] = host_max
                lib.check(lib.zk_confidential_verify_batch(pvk._h, n, xts, None, ptr(epochs), 32, ptr(ok), None))
            return run
        return ok, [("a_inputs_ready", a), ("b_host", entry("1000000000")), ("c_device", entry("0")), ("d_default", entry(None))]

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

    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-only":
        n = int(sys.argv[2])
        ok, runs = forms(n)
        for _ in range(5):
            runs[2][1]()
            assert ok.all()
        print("form (c), %d transactions, 5 calls" % n)
        return

    out = {"probe": "xt_verify", "host_threads": HOST_THREADS, "distinct": DISTINCT, "blocks": {}, "into_xy": {}}
    for n in (1, 64, 1024, 4096):
        ok, runs = forms(n)

        def check():
            assert ok.all(), "a transaction of the block was not accepted"
            ok[:] = 0
        res = timed(runs, check)
        fl = res["a_inputs_ready"]["median_ms"]
        res["b_minus_a_ms"] = round(res["b_host"]["median_ms"] - fl, 4)
        res["c_minus_a_ms"] = round(res["c_device"]["median_ms"] - fl, 4)
        res["d_minus_a_ms"] = round(res["d_default"]["median_ms"] - fl, 4)
        out["blocks"][str(n)] = res
    # IntoXY alone: the crossover of its two forms
    for npts in (1, 4, 8, 16, 32, 64, 128, 256, 704, 11264, 45056):
        pts = np.frombuffer(b"".join(points[i % len(points)] for i in range(npts)), dtype=np.uint8).copy()
        xy, stt = np.zeros(npts * 64, dtype=np.uint8), np.ones(npts, dtype=np.uint8)

        def call(device, host_max):
            def run():
                os.environ["ZKAMD_INTO_XY_HOST_MAX"] = host_max
                lib.check(lib.zk_jubjub_into_xy(ptr(pts), npts, device, ptr(xy), ptr(stt)))
            return run

        def check():
            assert not stt.any()
            stt[:] = 1
        out["into_xy"][str(npts)] = timed([("host", call(-1, "0")), ("device", call(0, "0"))], check)
    os.environ.pop("ZKAMD_INTO_XY_HOST_MAX", None)
    pvk.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
