#!/usr/bin/env python3
"""What a block of confidential transfers costs a validator, two ways, in one process: ONE JSON line.

  execute   zk_confidential_block_execute: signatures, rollovers, nonce pool, public inputs, proofs, balance updates in one call
  sequence  the four entries INTEGRATION.md 8.13 prescribes, one after another:
              1. zk_elgamal_ledger_apply with before_out  (the balance every extrinsic meets)
              2. zk_confidential_verify_batch             (enc_balances = the before_out of each first subtraction)
              3. zk_redjubjub_verify_batch
              4. zk_elgamal_ledger_apply again            (skip on the rejected: the state to store)

Honest blocks of n = 1, 32, 256, 1024, 4096 transfers: n accounts, every one due for rollover, account i sends to account i + 1,
every encoding of the block distinct, every proof forged for its inputs with the trapdoor of a small 22-input key
(tests/xt_verify_cases.py), every signature made by zk_redjubjub_sign.  The two ways are taken in turn inside every repetition;
three warm repetitions are discarded, then median, min and max of seven (host clock around the entries, each of which ends in a
device synchronise).  Both must accept everything and end in the same accounts.  One further repetition of each runs under
zk_profile_*: the per-stage totals of the device's work.

Forging proofs in Python takes about 20 ms each: `--blocks FILE` keeps the blocks in FILE (made when it is missing, which needs
no GPU), `--make-only` stops there.
Usage: python tools/block_probe.py [--blocks FILE] [--make-only] [--sizes 1,32,...] [out.json]
"""
import ctypes as C
import json
import os
import pickle
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1, 32, 256, 1024, 4096)
HOST_THREADS = 16
WARM, REPS = 3, 7
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
STAGES = ("into_xy", "block_gather", "ledger_scan", "block_balance_xy", "ledger_encode", "rj_decode", "rj_check", "verify_decode", "verify_decode_g1",
          "verify_prepare", "verify_rlc_scale", "verify_inputs", "verify_miller", "verify_final")
SUB, SKIP = 1, 2


def make_block(n, host_lib):
    """an honest block: dict of bytes, all of it what a caller of either way holds"""
    import zero_chain_amd as zk
    from oracle import jubjub as jj
    import xt_verify_cases as xc
    P, vkb = xc.small_conf_key()
    g = jj.note_commitment_randomness_generator()
    pts = [xc.prime_order_points()[0]]
    for _ in range(11 * n):
        pts.append(jj.add(pts[-1], g))
    enc = [jj.write_point(p) for p in pts]
    ge_enc = zk.g_epoch(0, lib=host_lib)
    ge = jj.read_point(ge_enc)
    sks = [(0x9e3779b97f4a7c15 * (i + 1) + n) % FS_MODULUS for i in range(n)]
    rvks = zk.jubjub_base_mul(sks, lib=host_lib)
    rvk_pts = [jj.read_point(bytes(b)) for b in rvks]
    msgs = [b"transfer %d of %d" % (i, n) for i in range(n)]
    sigs = zk.redjubjub_sign(sks, [bytes([i % 251]) * 80 for i in range(n)], msgs, lib=host_lib)
    # account i: key 11 i, balance 11 i + 1, + 2, pending + 3, + 4; extrinsic i: amounts + 5, + 6, fee + 7, randomness + 8, nonce + 9
    accounts = [dict(enc_key=enc[11 * i], balance=(enc[11 * i + 1], enc[11 * i + 2]), pending=(enc[11 * i + 3], enc[11 * i + 4]), flags=1) for i in range(n)]
    xts = []
    for i in range(n):
        r = (i + 1) % n
        met = [jj.add(pts[11 * i + 1], pts[11 * i + 3]), jj.add(pts[11 * i + 2], pts[11 * i + 4])]   # rolled over, nothing sent yet
        fields = [pts[11 * i], pts[11 * r], pts[11 * i + 5], pts[11 * i + 6], pts[11 * i + 8], pts[11 * i + 7], met[0], met[1], rvk_pts[i], ge, pts[11 * i + 9]]
        inputs = [c for p in fields for c in p]
        xts.append(dict(proof=xc.trapdoor_proof(P, inputs), enc_key_sender=enc[11 * i], enc_key_recipient=enc[11 * r], left_amount_sender=enc[11 * i + 5],
                        left_amount_recipient=enc[11 * i + 6], left_fee=enc[11 * i + 7], right_randomness=enc[11 * i + 8], rsk=bytes(32), rvk=bytes(rvks[i]),
                        enc_balance=bytes(64), nonce=enc[11 * i + 9]))
    return dict(n=n, vk=vkb, g_epoch=ge_enc, accounts=accounts, xts=xts, sigs=sigs, msgs=msgs)


def load_blocks(path, sizes):
    blocks = {}
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            blocks = pickle.load(f)
    missing = [n for n in sizes if n not in blocks]
    if missing:
        from zero_chain_amd import _lib as zl
        host_lib = zl.ZkLib(zl.LIB_PATH)   # (only entries that never touch the device)
        for n in missing:
            t0 = time.time()
            blocks[n] = make_block(n, host_lib)
            print("made the block of %d in %.1f s" % (n, time.time() - t0), file=sys.stderr, flush=True)
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
    out = {"probe": "block", "host_threads": HOST_THREADS, "warm": WARM, "reps": REPS, "sizes": {}}
    for n in sizes:
        blk = blocks[n]
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
        vks = u8(b"".join(x["rvk"] for x in blk["xts"]))
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(m) for m in blk["msgs"]])
        verdicts, stats = (zl.BlockVerdict * n)(), zl.BlockStats()
        results = {}

        def execute():
            lib.check(lib.zk_confidential_block_execute(pvk._h, n, xts, ptr(sigs), ptr(msgs), ptr(offs), n, acc, 0, None, ptr(ge), acc_out, verdicts,
                                                        C.byref(stats)))

        def check_execute():   # (outside the clock: walking ctypes structures costs Python microseconds per extrinsic)
            v = np.frombuffer(verdicts, dtype=np.uint8).reshape(n, 4)
            assert not v[:, 0].any() and stats.rounds == 1 and stats.proofs_verified == n, "the block is not honest"
            a = np.frombuffer(acc_out, dtype=np.uint8).reshape(n, C.sizeof(zl.BlockAccount))
            assert (a[:, 160] == 3).all(), "an account was not rolled over"
            results["execute"] = a[:, 32:160].tobytes()

        # the sequence's inputs, as INTEGRATION.md 8.13 maps a block: the pending slot of a rolled account starts as zero
        zero = b"\x01" + bytes(31)
        slots = u8(b"".join(a["balance"][0] + a["balance"][1] + zero + zero for a in blk["accounts"]))
        ops = (zl.LedgerOp * (5 * n))()
        rolled, k, first_sub = set(), 0, []
        for i, x in enumerate(blk["xts"]):
            for a in (i, (i + 1) % n):
                if a not in rolled:
                    rolled.add(a)
                    ops[k].slot, ops[k].flags = 2 * a, 0
                    ops[k].left[:], ops[k].right[:] = blk["accounts"][a]["pending"]
                    k += 1
            first_sub.append(k)
            for slot, flags, left in ((2 * i, SUB, "left_amount_sender"), (2 * i, SUB, "left_fee"), (2 * ((i + 1) % n) + 1, 0, "left_amount_recipient")):
                ops[k].slot, ops[k].flags = slot, flags
                ops[k].left[:], ops[k].right[:] = x[left], x["right_randomness"]
                k += 1
        n_ops = k
        slots_out, before = np.zeros(128 * n, dtype=np.uint8), np.zeros(64 * n_ops, dtype=np.uint8)
        slot_st, op_st = np.zeros(2 * n, dtype=np.uint8), np.zeros(n_ops, dtype=np.uint8)
        ok, refusal, sig_ok = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        idx = np.array(first_sub)

        def sequence():
            lib.check(lib.zk_elgamal_ledger_apply(2 * n, ptr(slots), n_ops, ops, 0, ptr(slots_out), ptr(before), ptr(slot_st), ptr(op_st)))
            bal = np.ascontiguousarray(before.reshape(n_ops, 64)[idx])
            lib.check(lib.zk_confidential_verify_batch(pvk._h, n, xts, ptr(bal), ptr(ge), 0, ptr(ok), ptr(refusal)))
            lib.check(lib.zk_redjubjub_verify_batch(n, ptr(vks), ptr(sigs), ptr(msgs), ptr(offs), 0, ptr(sig_ok), None))
            for i in np.nonzero((ok & sig_ok) == 0)[0]:
                for j in range(first_sub[i], first_sub[i] + 3):
                    ops[j].flags |= SKIP
            lib.check(lib.zk_elgamal_ledger_apply(2 * n, ptr(slots), n_ops, ops, 0, ptr(slots_out), None, ptr(slot_st), ptr(op_st)))

        def check_sequence():
            assert ok.all() and sig_ok.all() and not refusal.any(), "the block is not honest"
            results["sequence"] = slots_out.tobytes()

        runs = (("execute", execute, check_execute), ("sequence", sequence, check_sequence))
        walls = {name: [] for name, _, _ in runs}
        for rep in range(WARM + REPS):
            for name, fn, check in runs:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                check()
                if rep >= WARM:
                    walls[name].append(dt)
            assert results["execute"] == results["sequence"], "the two ways end in different accounts"
        row = {name: {"median_ms": round(statistics.median(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)} for name, w in walls.items()}
        for name, fn, _ in runs:
            with zk.KernelTimer(lib) as t:
                fn()
                row[name]["stages_ms"] = {s: [c, round(ms, 4)] for s in STAGES for c, ms in [t.get(s)] if c}
        row["points_decoded"], row["n_ops"] = stats.points_decoded, n_ops
        row["execute_slowest_below_sequence_fastest"] = row["execute"]["max_ms"] < row["sequence"]["min_ms"]
        out["sizes"][str(n)] = row
        pvk.close()
    line = json.dumps(out)
    print(line)
    if args:
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
