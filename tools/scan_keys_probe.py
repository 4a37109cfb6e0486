#!/usr/bin/env python3
"""What reading a block with a SET of K decryption keys costs in one call (zk_confidential_scan_keys / zk_anonymous_scan_keys),
beside the loop of K single-key calls it replaces: ONE JSON line.

  confidential: blocks of 1024 extrinsics (random amounts below 10^6, zeroed proofs, limit 10^6) in two shapes
    all        every party is a key of the set, sender and recipient distinct where K > 1: 2048 hits (1024 at K = 1, role 3)
    sixteenth  one extrinsic in sixteen is such a transfer, the others are between strangers: 128 hits (64 at K = 1)
  for K in 1, 4, 16, 64, 256, 1024.  Per shape and K, wall ms (host clock around the entry, which ends in a device synchronise;
  one warm repetition discarded, median of five with min and max, the four taken in turn inside every repetition):
    host      ZKAMD_SCAN_HOST_MAX huge: decoding and dk * right once per hit on the host threads, one upload, the search
    device    ZKAMD_SCAN_HOST_MAX=0: k_keys_points + k_scan_combine, then the search on the resident rows
    default   the variable unset
    loop      K calls of zk_confidential_scan on the same block, one per key, the variable unset
  the device time of the stages (HIP events, zk_profile_*) in a run of their own in the device form, and the wall time of
  zk_scan_keys_create for the K keys.
  anonymous: 1024 rings whose twelve members are all keys of a set of 64 (12 288 hits), the same four columns.
Usage: python tools/scan_keys_probe.py [out.json]
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

N = 1024
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
ENV = "ZKAMD_SCAN_HOST_MAX"
LIMIT = 1000000
STAGES = ("keys_points", "scan_combine", "elgamal_dlog")


def main():
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = random.Random(18)
    fs = lambda: rng.randrange(1, FS_MODULUS)
    all_dks = [fs() for _ in range(1024)]
    all_enc = zk.jubjub_base_mul(all_dks, lib=lib)
    strangers = zk.jubjub_base_mul([fs() for _ in range(12)], lib=lib)

    def timed(runs, check, warm=1, reps=5):
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

    def confidential_block(k, every):
        """(xts, [(xt, key, role, amount)] in hit order): `every`-th extrinsics are transfers inside the set of the first k keys"""
        parties, amounts, want = [], [], []
        for i in range(N):
            a = rng.randrange(LIMIT)
            amounts.append(a)
            if i % every:
                parties.append((None, None))
                continue
            s = rng.randrange(k)
            r = s if k == 1 else (s + 1 + rng.randrange(k - 1)) % k
            parties.append((s, r))
            want += [(i, s, 3, a)] if s == r else sorted([(i, s, 1, a), (i, r, 2, a)])
        key = lambda p, other: all_enc[p] if p is not None else strangers[other]
        rnd = [fs() for _ in range(N)]
        ls, right = zk.elgamal_encrypt(amounts, rnd, [key(s, 0) for s, _ in parties], lib=lib)
        lr, _ = zk.elgamal_encrypt(amounts, rnd, [key(r, 1) for _, r in parties], lib=lib)
        lf, _ = zk.elgamal_encrypt([1] * N, rnd, [key(s, 0) for s, _ in parties], lib=lib)
        xts = (_lib.ConfidentialXt * N)()
        for i, x in enumerate(xts):
            x.enc_key_sender[:], x.enc_key_recipient[:] = key(parties[i][0], 0), key(parties[i][1], 1)
            x.left_amount_sender[:], x.left_amount_recipient[:], x.left_fee[:], x.right_randomness[:] = ls[i], lr[i], lf[i], right[i]
        return xts, want

    def measure(k, xts, want, scan_keys_fn, scan_fn, hit_type, result_type, hit_ok, result_ok):
        """the four columns, the stages and the creation time for one block and the first k keys"""
        kb = np.frombuffer(b"".join(dk.to_bytes(32, "little") for dk in all_dks[:k]), dtype=np.uint8).copy()
        creates = []
        for _ in range(6):
            h = C.c_void_p()
            t0 = time.perf_counter()
            lib.check(lib.zk_scan_keys_create(ptr(kb), k, C.byref(h)))
            creates.append((time.perf_counter() - t0) * 1e3)
            lib.zk_scan_keys_free(h)
        keys = zk.ScanKeys(all_dks[:k], lib=lib)
        hits, count = (hit_type * len(want))(), C.c_size_t(0)
        res = (result_type * N)()
        mine = {}
        for w in want:
            mine.setdefault(w[1], []).append(w)
        kptr = [C.c_void_p(kb.ctypes.data + 32 * key) for key in range(k)]

        def one_call():
            lib.check(scan_keys_fn(table._h, keys._h, N, xts, LIMIT, hits, len(want), C.byref(count)))

        def loop():   # (the calls alone: what they write is checked once, outside the clock, below)
            for key in range(k):
                lib.check(scan_fn(table._h, N, xts, kptr[key], LIMIT, res))

        def check(name):
            if name != "loop":
                assert count.value == len(want) and all((h.xt, h.key) == w[:2] and hit_ok(h.r, w) for h, w in zip(hits, want)), name
                C.memset(hits, 0, C.sizeof(hits))
                count.value = 0
        try:
            os.environ.pop(ENV, None)
            for key in range(k):
                lib.check(scan_fn(table._h, N, xts, kptr[key], LIMIT, res))
                raw = bytes(res)
                assert all(result_ok(res[w[0]], w) for w in mine.get(key, ())) and \
                    sum(1 for i in range(N) if raw[16 * i:16 * i + 16] != bytes(16)) == len(mine.get(key, ())), "the single-key loop: a wrong result"
            row = timed([("host", with_env("1000000000", one_call)), ("device", with_env("0", one_call)), ("default", with_env(None, one_call)),
                         ("loop", with_env(None, loop))], check)
            os.environ[ENV] = "0"
            with zk.KernelTimer(lib) as kt:
                one_call()
                row["device_stages_ms"] = {s: round(kt.get(s)[1], 4) for s in STAGES}
        finally:
            keys.close()
        row["hits"] = len(want)
        row["create_ms"] = {"median_ms": round(statistics.median(creates[1:]), 4), "min_ms": round(min(creates[1:]), 4), "max_ms": round(max(creates[1:]), 4)}
        return row

    out = {"probe": "scan_keys", "host_threads": HOST_THREADS, "extrinsics": N, "limit": LIMIT, "confidential": {"all": {}, "sixteenth": {}}, "anonymous": {}}
    table = zk.ElGamalTable(lib=lib)
    try:
        c_hit = lambda r, w: (r.role, r.refusal) == (w[2], 0) and r.found == (3 if w[2] & 1 else 0) | (4 if w[2] & 2 else 0) and \
            (r.amount_sent, r.fee) == ((w[3], 1) if w[2] & 1 else (0, 0)) and r.amount_received == (w[3] if w[2] & 2 else 0)
        for shape, every in (("all", 1), ("sixteenth", 16)):
            for k in (1, 4, 16, 64, 256, 1024):
                print("confidential", shape, "K =", k, file=sys.stderr, flush=True)
                xts, want = confidential_block(k, every)
                out["confidential"][shape][str(k)] = measure(k, xts, want, lib.zk_confidential_scan_keys, lib.zk_confidential_scan,
                                                             _lib.ConfidentialScanHit, _lib.ConfidentialScanResult, c_hit, c_hit)
        k = 64
        amounts = [rng.randrange(LIMIT) for _ in range(N)]
        rnd = [fs() for _ in range(N)]
        rings = [rng.sample(range(k), 12) for _ in range(N)]
        lefts, rights = zk.elgamal_encrypt([amounts[i] if p == 1 else 0 for i in range(N) for p in range(12)], [rnd[i] for i in range(N) for _ in range(12)],
                                           [all_enc[m] for ring in rings for m in ring], lib=lib)
        la, ra = zk.elgamal_encrypt(amounts, [0] * N, [all_enc[ring[0]] for ring in rings], lib=lib)     # position 0 sends, position 1 receives
        minus, _ = zk.elgamal_add([lefts[12 * i] for i in range(N)], [rights[12 * i] for i in range(N)], la, ra, subtract=True, lib=lib)
        xts = (_lib.AnonymousXt * N)()
        want = []
        for i, x in enumerate(xts):
            for p in range(12):
                x.enc_keys[p][:], x.left_ciphertexts[p][:] = all_enc[rings[i][p]], (minus[i] if p == 0 else lefts[12 * i + p])
            x.right_ciphertext[:] = rights[12 * i]
            want += sorted((i, m, 1 << p, (-amounts[i], amounts[i])[p] if p < 2 else 0) for p, m in enumerate(rings[i]))
        a_hit = lambda r, w: (r.members, r.found, r.refusal, r.delta) == (w[2], 1, 0, w[3])
        out["anonymous"]["%d" % k] = measure(k, xts, want, lib.zk_anonymous_scan_keys, lib.zk_anonymous_scan, _lib.AnonymousScanHit,
                                             _lib.AnonymousScanResult, a_hit, a_hit)
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
