#!/usr/bin/env python3
"""What a block of encrypted-asset extrinsics costs a validator, in one process: ONE JSON line.

  transfers  a transfer-only single-asset block at n = 64, 256, 1024 through zk_asset_block_execute, beside
             zk_confidential_block_execute on the same block (tools/block_probe.py's honest blocks: n accounts, all due, account i
             sends to account i + 1) - the like-for-like: the same work, the scan that can forget in place of the ledger's
  mixed      the block of 1024 with one issue and one destroy in every 32 extrinsics (extrinsic i with i % 32 == 7 an issue by
             account i's key, with i % 32 == 23 a destroy of account i), all accepted in one round, with the per-stage totals of
             zk_profile_*

The entries are taken in turn inside every repetition, the order swapped from one repetition to the next so that neither
always follows the other; two warm repetitions are discarded, then median, min and max of five
(host clock around the entries, each of which ends in a device synchronise).  Both entries must accept everything and, on the
transfer-only block, end in the same accounts.

Forging proofs in Python takes about 20 ms each: `--blocks FILE` keeps the blocks in FILE (made when it is missing, which needs
no GPU), `--make-only` stops there.
Usage: python tools/asset_block_probe.py [--blocks FILE] [--make-only] [--sizes 64,256,...] [out.json]
"""
import ctypes as C
import importlib.util
import json
import os
import pickle
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (64, 256, 1024)
MIXED = 1024
HOST_THREADS = 16
WARM, REPS = 2, 5
ASSET = 3
STAGES = ("into_xy", "block_gather", "ledger_scan", "block_balance_xy", "ledger_encode", "asset_scan", "asset_balance_xy", "asset_encode", "rj_decode", "rj_check",
          "verify_decode", "verify_decode_g1", "verify_prepare", "verify_rlc_scale", "verify_inputs", "verify_miller", "verify_final")


def _block_probe():
    spec = importlib.util.spec_from_file_location("block_probe", os.path.join(ROOT, "tools", "block_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_mixed(blk):
    """the honest block with every 32nd extrinsic turned into an issue and another into a destroy, their proofs forged anew"""
    from oracle import jubjub as jj
    import xt_verify_cases as xc
    P, _ = xc.small_conf_key()
    pt = lambda enc: jj.read_point(bytes(enc))
    g = jj.note_commitment_randomness_generator()
    extra = jj.mul(g, 0x5eed)
    kinds, xts = [], []
    for i, x in enumerate(blk["xts"]):
        kind = {7: "issue", 23: "destroy"}.get(i % 32, "transfer")
        kinds.append(kind)
        if kind != "transfer":
            extra = jj.add(extra, g)
            x = dict(x, enc_balance=jj.write_point(extra) + x["left_amount_recipient"])
            fields = [x["enc_key_sender"], x["enc_key_sender"], x["left_amount_sender"], x["left_amount_sender"], x["right_randomness"], x["left_fee"],
                      x["enc_balance"][:32], x["enc_balance"][32:], x["rvk"], blk["g_epoch"], x["nonce"]]
            x["proof"] = xc.trapdoor_proof(P, [c for f in fields for c in pt(f)])
        xts.append(x)
    return dict(blk, xts=xts, kinds=kinds)


def load_blocks(path, sizes):
    blocks = {}
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            blocks = pickle.load(f)
    missing = [n for n in tuple(sizes) + ("mixed",) if n not in blocks]
    if missing:
        from zero_chain_amd import _lib as zl
        host_lib = zl.ZkLib(zl.LIB_PATH)   # (only entries that never touch the device)
        bp = _block_probe()
        for n in missing:
            t0 = time.time()
            blocks[n] = make_mixed(blocks[MIXED] if MIXED in blocks else bp.make_block(MIXED, host_lib)) if n == "mixed" else bp.make_block(n, host_lib)
            print("made the block %s in %.1f s" % (n, time.time() - t0), file=sys.stderr, flush=True)
        if path:
            with open(path, "wb") as f:
                pickle.dump(blocks, f)
    return blocks


def main():
    args = sys.argv[1:]
    path, make_only, sizes = None, False, SIZES
    while args and args[0].startswith("--"):
        a = args.pop(0)
        if a == "--blocks":
            path = args.pop(0)
        elif a == "--make-only":
            make_only = True
        elif a == "--sizes":
            sizes = tuple(int(v) for v in args.pop(0).split(","))
    blocks = load_blocks(path, sizes)
    if make_only:
        return
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib as zl
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8).copy()
    out = {"probe": "asset_block", "host_threads": HOST_THREADS, "warm": WARM, "reps": REPS, "sizes": {}}
    for key in tuple(sizes) + ("mixed",):
        blk = blocks[key]
        n = blk["n"]
        kinds = blk.get("kinds") or ["transfer"] * n
        pvk = zk.prepare_verifying_key(blk["vk"], lib=lib)
        xts = (zl.ConfidentialXt * n)()
        for dst, x in zip(xts, blk["xts"]):
            for f in zk.XT_FIELDS:
                getattr(dst, f)[:] = x[f]
        acc, acc_out = (zl.BlockAccount * n)(), (zl.BlockAccount * n)()
        for dst, a in zip(acc, blk["accounts"]):
            dst.enc_key[:] = a["enc_key"]
            dst.balance[:] = a["balance"][0] + a["balance"][1]
            dst.pending[:] = a["pending"][0] + a["pending"][1]
            dst.flags = a["flags"]
        sigs, msgs, ge = u8(b"".join(blk["sigs"])), u8(b"".join(blk["msgs"])), u8(blk["g_epoch"])
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(m) for m in blk["msgs"]])
        kb = np.array([zk.ASSET_KINDS.index(k) for k in kinds], dtype=np.uint8)
        ids, acc_ids = np.full(n, ASSET, dtype=np.uint32), np.full(n, ASSET, dtype=np.uint32)
        verdicts, stats, effects, next_out = (zl.BlockVerdict * n)(), zl.BlockStats(), (zl.AssetEffect * n)(), C.c_uint32(0)
        results = {}
        n_issue, n_destroy = kinds.count("issue"), kinds.count("destroy")

        def asset():
            lib.check(lib.zk_asset_block_execute(pvk._h, n, xts, ptr(kb), ptr(ids), ptr(sigs), ptr(msgs), ptr(offs), n, acc, ptr(acc_ids), 0, None, ptr(ge), 10,
                                                 acc_out, verdicts, effects, C.byref(next_out), C.byref(stats)))

        def confidential():
            lib.check(lib.zk_confidential_block_execute(pvk._h, n, xts, ptr(sigs), ptr(msgs), ptr(offs), n, acc, 0, None, ptr(ge), acc_out, verdicts,
                                                        C.byref(stats)))

        def check(name):   # (outside the clock)
            v = np.frombuffer(verdicts, dtype=np.uint8).reshape(n, 4)
            assert not v[:, 0].any() and stats.rounds == 1 and stats.proofs_verified == n, "the block is not honest"
            a = np.frombuffer(acc_out, dtype=np.uint8).reshape(n, C.sizeof(zl.BlockAccount))
            if name == "asset":
                assert next_out.value == 10 + n_issue and int((a[:, 160] & 4 != 0).sum()) == n_destroy
            results[name] = a[:, 32:161].tobytes()
            results["points_decoded_" + name] = stats.points_decoded

        runs = (("asset", asset),) if key == "mixed" else (("asset", asset), ("confidential", confidential))
        walls = {name: [] for name, _ in runs}
        for rep in range(WARM + REPS):
            for name, fn in (runs if rep % 2 == 0 else runs[::-1]):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                check(name)
                if rep >= WARM:
                    walls[name].append(dt)
            assert key == "mixed" or results["asset"] == results["confidential"], "the two entries end in different accounts"
        row = {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4), "runs_ms": [round(v, 4) for v in w]}
               for name, w in walls.items()}   # (runs_ms in order: the asset entry came first in runs 0, 2 and 4, second in 1 and 3)
        for name, fn in runs:
            with zk.KernelTimer(lib) as t:
                fn()
                row[name]["stages_ms"] = {s: [c, round(ms, 4)] for s in STAGES for c, ms in [t.get(s)] if c}
            row[name]["points_decoded"] = results["points_decoded_" + name]
        row["n"], row["issues"], row["destroys"] = n, n_issue, n_destroy
        if key != "mixed":
            row["asset_median_above_confidential_slowest"] = row["asset"]["median_ms"] > row["confidential"]["max_ms"]
        out["sizes"][str(key)] = row
        pvk.close()
    line = json.dumps(out)
    print(line)
    if args:
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
