#!/usr/bin/env python3
"""What deriving the children of one extended key costs in one call (zk_hd_derive, csrc/hd_keys.h): ONE JSON line.

  derive: the children 0 .. n - 1 of one xpgk, all three outputs, for n in 1, 64, 256, 1024, 4096, 16384, 65536.  Per n, wall ms
  (host clock around the entry, which ends in a device synchronise; one warm repetition discarded, median of five with min and max,
  the columns taken in turn inside every repetition):
    host      ZKAMD_HD_HOST_MAX huge: both multiplications of every child on the host threads, one batch_to_affine per thread
    device    ZKAMD_HD_HOST_MAX=0: k_hd_children, every lane loading its own table entries from global memory
    staged    the same with ZKAMD_HD_STAGE_TABLE=1: the block copies each window of the table into LDS first
    default   both variables unset
    hash      the xsk route with xkeys_out alone: the hashes every form shares, no point work
  and the device time of the stages (HIP events, zk_profile_*: hd_upload, hd_children, hd_download) in runs of their own for the
  two table-read variants.
  scan_keys: zk_scan_keys_create_hd (default form) beside host-form zk_hd_derive + zk_scan_keys_create on the same indices.
Usage: python tools/hd_probe.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 64, 256, 1024, 4096, 16384, 65536)
HOST_THREADS = 16   # the host form's pool: the cores a process gets on the measurement box
HOST_MAX, STAGE = "ZKAMD_HD_HOST_MAX", "ZKAMD_HD_STAGE_TABLE"
STAGES = ("hd_upload", "hd_children", "hd_download")


def main():
    import numpy as np
    import zero_chain_amd as zk
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    xsk = zk.hd_master(bytes(range(32)), lib=lib)
    xpgk = zk.hd_xpgk(xsk, lib=lib)
    xsk_b, xpgk_b = C.create_string_buffer(xsk, 73), C.create_string_buffer(xpgk, 73)

    def timed(runs, warm=1, reps=5):
        walls = {name: [] for name, _ in runs}
        for rep in range(warm + reps):
            for name, fn in runs:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= warm:
                    walls[name].append(dt)
        return {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)} for name, w in walls.items()}

    def with_env(host_max, stage, fn):
        def run():
            for name, value in ((HOST_MAX, host_max), (STAGE, stage)):
                if value is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = value
            fn()
        return run

    out = {"probe": "hd", "host_threads": HOST_THREADS, "derive": {}, "scan_keys": {}}
    try:
        for n in SIZES:
            print("n =", n, file=sys.stderr, flush=True)
            idx = np.arange(n, dtype=np.uint32)
            xk, dk, ek = np.zeros(73 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
            seen = {}

            def derive(name):
                def run():
                    lib.check(lib.zk_hd_derive(zk.HD_XPGK, xpgk_b, ptr(idx), n, 0, ptr(xk), ptr(dk), ptr(ek)))
                    seen[name] = (xk.tobytes(), dk.tobytes(), ek.tobytes())
                return run

            def hash_only():
                lib.check(lib.zk_hd_derive(zk.HD_XSK, xsk_b, ptr(idx), n, 0, ptr(xk), None, None))

            row = timed([("host", with_env("1000000000", None, derive("host"))), ("device", with_env("0", None, derive("device"))),
                         ("staged", with_env("0", "1", derive("staged"))), ("default", with_env(None, None, derive("default"))),
                         ("hash", with_env(None, None, hash_only))])
            assert seen["host"] == seen["device"] == seen["staged"] == seen["default"], "the forms disagree at n = %d" % n
            for name, stage in (("device", None), ("staged", "1")):
                with zk.KernelTimer(lib) as kt:
                    with_env("0", stage, derive(name))()
                    row[name]["stages_ms"] = {s: round(kt.get(s)[1], 4) for s in STAGES}
            out["derive"][str(n)] = row

            def create_hd():
                h = C.c_void_p()
                lib.check(lib.zk_scan_keys_create_hd(zk.HD_XPGK, xpgk_b, ptr(idx), n, 0, C.byref(h)))
                lib.zk_scan_keys_free(h)

            def derive_then_create():
                lib.check(lib.zk_hd_derive(zk.HD_XPGK, xpgk_b, ptr(idx), n, 0, None, ptr(dk), None))
                h = C.c_void_p()
                lib.check(lib.zk_scan_keys_create(ptr(dk), n, C.byref(h)))
                lib.zk_scan_keys_free(h)

            out["scan_keys"][str(n)] = timed([("create_hd", with_env(None, None, create_hd)),
                                              ("host_derive_then_create", with_env("1000000000", None, derive_then_create))])
    finally:
        os.environ.pop(HOST_MAX, None)
        os.environ.pop(STAGE, None)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
