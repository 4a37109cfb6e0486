#!/usr/bin/env python3
"""What the balances of the accounts of a key set cost in one call (zk_balance_keys), beside the route a caller had before it on
the same accounts in the same process - one zk_elgamal_add call of n pairs, then one zk_elgamal_decrypt call of n: ONE JSON line.

  accounts of n = 1, 64, 256, 1024 and 4096 keys, one account per key, all matching, all due, balance and pending non-zero and
  their sum below 10^6; limits 10^6 and 2^32.  Per n and limit, wall ms (host clock around the entry, which ends in a device
  synchronise; two warm repetitions discarded, median of seven with min and max, the four taken in turn inside every repetition):
    host       ZKAMD_SCAN_HOST_MAX huge: decoding, the sums and dk * right once per hit on the host threads, one upload, the search
    device     ZKAMD_SCAN_HOST_MAX=0: k_keys_points + k_balance_combine, then the search on the resident rows
    default    the variable unset
    two_calls  zk_elgamal_add, then zk_elgamal_decrypt with one key per ciphertext
  and the device time of the stages (HIP events, zk_profile_*) in a run of their own in the device form.
Usage: python tools/balance_probe.py [out.json]     (the committed run: profiles/r21_balance_probe.json)
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

SIZES = (1, 64, 256, 1024, 4096)
LIMITS = (1000000, 1 << 32)
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
ENV = "ZKAMD_SCAN_HOST_MAX"
STAGES = ("keys_points", "balance_combine", "elgamal_dlog")
WARM, REPS = 2, 7


def main():
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = random.Random(21)
    n_max = max(SIZES)
    dks = [rng.randrange(1, FS_MODULUS) for _ in range(n_max)]
    enc = zk.jubjub_base_mul(dks, lib=lib)
    balance = [rng.randrange(1, 500000) for _ in range(n_max)]
    pending = [rng.randrange(1, 500000) for _ in range(n_max)]
    bl, br = zk.elgamal_encrypt(balance, [rng.randrange(1, FS_MODULUS) for _ in range(n_max)], enc, lib=lib)
    pl, pr = zk.elgamal_encrypt(pending, [rng.randrange(1, FS_MODULUS) for _ in range(n_max)], enc, lib=lib)
    accounts = (_lib.BlockAccount * n_max)()
    for i, a in enumerate(accounts):
        a.enc_key[:], a.balance[:], a.pending[:], a.flags = enc[i], bl[i] + br[i], pl[i] + pr[i], zk.BLOCK_ROLLOVER_DUE
    pack = lambda pts, n: np.frombuffer(b"".join(pts[:n]), dtype=np.uint8).copy()

    def with_env(host_max, fn):
        def run():
            if host_max is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = host_max
            fn()
        return run

    out = {"probe": "balance", "host_threads": HOST_THREADS, "warm": WARM, "reps": REPS, "sizes": {}}
    table = zk.ElGamalTable(lib=lib)
    try:
        for n in SIZES:
            keys = zk.ScanKeys(dks[:n], lib=lib)
            kb = np.frombuffer(b"".join(dk.to_bytes(32, "little") for dk in dks[:n]), dtype=np.uint8).copy()
            ins = [pack(p, n) for p in (bl, br, pl, pr)]
            sl, sr = np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
            values, found = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
            hits, count = (_lib.BalanceHit * n)(), C.c_size_t(0)
            want = [balance[i] + pending[i] for i in range(n)]
            try:
                for limit in LIMITS:
                    print("n =", n, "limit =", limit, file=sys.stderr, flush=True)

                    def one_call():
                        lib.check(lib.zk_balance_keys(table._h, keys._h, n, accounts, limit, hits, n, C.byref(count)))

                    def two_calls():
                        lib.check(lib.zk_elgamal_add(*[ptr(a) for a in ins], n, 0, ptr(sl), ptr(sr)))
                        lib.check(lib.zk_elgamal_decrypt(table._h, n, ptr(sl), ptr(sr), ptr(kb), 32, limit, ptr(values), ptr(found)))

                    def check(name):
                        if name == "two_calls":
                            assert found.all() and values.tolist() == want, name
                            totals = sl.tobytes(), sr.tobytes()
                            check.totals = [totals[0][32 * i:32 * i + 32] + totals[1][32 * i:32 * i + 32] for i in range(n)]
                            values[:] = 0
                            found[:] = 0
                        else:
                            assert count.value == n and all((h.account, h.key, h.r.found, h.r.refusal, h.r.value) == (i, i, 1, 0, want[i])
                                                            for i, h in enumerate(hits)), name
                            check.mine = [bytes(h.r.enc_total) for h in hits]
                            C.memset(hits, 0, C.sizeof(hits))
                            count.value = 0
                    runs = [("host", with_env("1000000000", one_call)), ("device", with_env("0", one_call)), ("default", with_env(None, one_call)),
                            ("two_calls", with_env(None, two_calls))]
                    walls = {name: [] for name, _ in runs}
                    for rep in range(WARM + REPS):
                        for name, fn in runs:
                            t0 = time.perf_counter()
                            fn()
                            dt = (time.perf_counter() - t0) * 1e3
                            check(name)
                            if rep >= WARM:
                                walls[name].append(dt)
                    assert check.mine == check.totals, "enc_total differs from zk_elgamal_add"
                    row = {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)} for name, w in walls.items()}
                    os.environ[ENV] = "0"
                    with zk.KernelTimer(lib) as kt:
                        one_call()
                        row["device_stages_ms"] = {s: round(kt.get(s)[1], 4) for s in STAGES}
                    os.environ.pop(ENV, None)
                    out["sizes"].setdefault(str(n), {})[str(limit)] = row
            finally:
                keys.close()
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
