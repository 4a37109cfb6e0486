#!/usr/bin/env python3
"""What a block of anonymous transfers costs a validator, two ways, in one process: ONE JSON line.

  execute   zk_anonymous_block_execute: signatures, rollovers, nonce pool, public inputs, proofs, pending transfers in one call
  sequence  the four entries a runtime calls without it, one after another:
              1. zk_redjubjub_verify_batch
              2. zk_elgamal_ledger_apply for the rollovers  (slots: the balances; ops: the pending transfer of every due account
                                                             a dispatched extrinsic names; the rolled balances are the slots'
                                                             outputs, so before_out is not asked for: the leanest form)
              3. zk_anonymous_verify_batch                  (enc_balances = the twelve rolled balances of each ring)
              4. zk_elgamal_ledger_apply again              (slots: the pending transfers after rollover; ops: twelve additions
                                                             per extrinsic, skip on the rejected)

Honest blocks of n = 1, 8, 64, 256, 1024 extrinsics over 4 n + 8 accounts, every one due for rollover; ring i is accounts
4 i .. 4 i + 11, so neighbouring rings share eight members as overlapping anonymity sets do.  Every other encoding of the block is
distinct, every proof is forged for its 104 inputs with the trapdoor of a small key (tests/xt_verify_cases.py), every signature
made by zk_redjubjub_sign.  The two ways are taken in turn inside every repetition; two warm repetitions are discarded, then
median, min and max of five (host clock around the entries, each of which ends in a device synchronise).  Both must accept
everything and end in the same accounts.  One further repetition of each runs under zk_profile_*: the per-stage totals of the
device's work.

Forging proofs in Python takes about 25 ms each: `--blocks FILE` keeps the blocks in FILE (made when it is missing, which needs
no GPU), `--make-only` stops there.
Usage: python tools/anon_block_probe.py [--blocks FILE] [--make-only] [--sizes 1,8,...] [out.json]
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

SIZES = (1, 8, 64, 256, 1024)
HOST_THREADS = 16
WARM, REPS = 2, 5
RING = 12
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
STAGES = ("into_xy", "block_gather", "ring_balance_xy", "ledger_scan", "ledger_encode", "rj_decode", "rj_check", "verify_decode", "verify_decode_g1",
          "verify_prepare", "verify_rlc_scale", "verify_inputs", "verify_miller", "verify_final")
SKIP = 2


def make_block(n, host_lib):
    """an honest block: dict of bytes, all of it what a caller of either way holds"""
    import zero_chain_amd as zk
    from oracle import jubjub as jj
    import helpers
    import xt_verify_cases as xc
    r1, asg, P, pk = helpers.small_case(32, 105, 6, 30)
    n_acc = 4 * n + 8
    g = jj.note_commitment_randomness_generator()
    pts = [xc.prime_order_points()[0]]
    for _ in range(5 * n_acc + 14 * n):
        pts.append(jj.add(pts[-1], g))
    enc = [jj.write_point(p) for p in pts]
    ge_enc = zk.g_epoch(0, lib=host_lib)
    ge = jj.read_point(ge_enc)
    sks = [(0x9e3779b97f4a7c15 * (i + 1) + n) % FS_MODULUS for i in range(n)]
    rvks = zk.jubjub_base_mul(sks, lib=host_lib)
    rvk_pts = [jj.read_point(bytes(b)) for b in rvks]
    msgs = [b"anonymous transfer %d of %d" % (i, n) for i in range(n)]
    sigs = zk.redjubjub_sign(sks, [bytes([i % 251]) * 80 for i in range(n)], msgs, lib=host_lib)
    # account a: key 5 a, balance 5 a + 1, + 2, pending + 3, + 4; extrinsic i, from x = 5 n_acc + 14 i: twelve lefts, the right, the nonce
    accounts = [dict(enc_key=enc[5 * a], balance=(enc[5 * a + 1], enc[5 * a + 2]), pending=(enc[5 * a + 3], enc[5 * a + 4]), flags=1) for a in range(n_acc)]
    met = [(jj.add(pts[5 * a + 1], pts[5 * a + 3]), jj.add(pts[5 * a + 2], pts[5 * a + 4])) for a in range(n_acc)]   # rolled over
    xts = []
    for i in range(n):
        x, ring = 5 * n_acc + 14 * i, range(4 * i, 4 * i + RING)
        fields = [pts[5 * a] for a in ring] + [pts[x + k] for k in range(RING)] + [met[a][0] for a in ring] + [met[a][1] for a in ring] + \
                 [pts[x + 12], rvk_pts[i], ge, pts[x + 13]]
        inputs = [c for p in fields for c in p]
        xts.append(dict(proof=xc.trapdoor_proof(P, inputs), enc_keys=[enc[5 * a] for a in ring], left_ciphertexts=[enc[x + k] for k in range(RING)],
                        right_ciphertext=enc[x + 12], nonce=enc[x + 13], rsk=bytes(32), rvk=bytes(rvks[i])))
    return dict(n=n, vk=xc.vk_bytes_of(pk), g_epoch=ge_enc, accounts=accounts, xts=xts, sigs=sigs, msgs=msgs)


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
    out = {"probe": "anon_block", "host_threads": HOST_THREADS, "warm": WARM, "reps": REPS, "sizes": {}}
    for n in sizes:
        blk = blocks[n]
        n_acc = len(blk["accounts"])
        pvk = zk.prepare_verifying_key(blk["vk"], lib=lib)
        xts = (zl.AnonymousXt * n)()
        for dst, x in zip(xts, blk["xts"]):
            for f in ("proof", "right_ciphertext", "nonce", "rsk", "rvk"):
                getattr(dst, f)[:] = x[f]
            for f in ("enc_keys", "left_ciphertexts"):
                for k in range(RING):
                    getattr(dst, f)[k][:] = x[f][k]
        acc, acc_out = (zl.BlockAccount * n_acc)(), (zl.BlockAccount * n_acc)()
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
            lib.check(lib.zk_anonymous_block_execute(pvk._h, n, xts, ptr(sigs), ptr(msgs), ptr(offs), n_acc, acc, 0, None, ptr(ge), acc_out, verdicts,
                                                     C.byref(stats)))

        def check_execute():   # (outside the clock: walking ctypes structures costs Python microseconds per extrinsic)
            v = np.frombuffer(verdicts, dtype=np.uint8).reshape(n, 4)
            assert not v[:, 0].any() and stats.rounds == 1 and stats.proofs_verified == n, "the block is not honest"
            a = np.frombuffer(acc_out, dtype=np.uint8).reshape(n_acc, C.sizeof(zl.BlockAccount))
            assert (a[:, 160] == 3).all(), "an account was not rolled over"
            results["execute"] = (a[:, 32:96].tobytes(), a[:, 96:160].tobytes())

        # the sequence's inputs: every account is due and named, so every one rolls over and its pending slot starts as zero
        zero = b"\x01" + bytes(31)
        bal_slots = u8(b"".join(a["balance"][0] + a["balance"][1] for a in blk["accounts"]))
        pen_slots = u8((zero + zero) * n_acc)
        roll_ops = (zl.LedgerOp * n_acc)()
        for a, src in enumerate(blk["accounts"]):
            roll_ops[a].slot, roll_ops[a].flags = a, 0
            roll_ops[a].left[:], roll_ops[a].right[:] = src["pending"]
        add_ops = (zl.LedgerOp * (RING * n))()
        ring_idx = np.zeros((n, RING), dtype=np.int64)
        for i, x in enumerate(blk["xts"]):
            for k in range(RING):
                o = add_ops[RING * i + k]
                o.slot, o.flags = 4 * i + k, 0
                o.left[:], o.right[:] = x["left_ciphertexts"][k], x["right_ciphertext"]
                ring_idx[i, k] = 4 * i + k
        bal_out, pen_out = np.zeros(64 * n_acc, dtype=np.uint8), np.zeros(64 * n_acc, dtype=np.uint8)
        slot_st, roll_st, add_st = np.zeros(n_acc, dtype=np.uint8), np.zeros(n_acc, dtype=np.uint8), np.zeros(RING * n, dtype=np.uint8)
        ok, refusal, sig_ok = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

        def sequence():
            lib.check(lib.zk_redjubjub_verify_batch(n, ptr(vks), ptr(sigs), ptr(msgs), ptr(offs), 0, ptr(sig_ok), None))
            lib.check(lib.zk_elgamal_ledger_apply(n_acc, ptr(bal_slots), n_acc, roll_ops, 0, ptr(bal_out), None, ptr(slot_st), ptr(roll_st)))
            bal = np.ascontiguousarray(bal_out.reshape(n_acc, 64)[ring_idx])
            lib.check(lib.zk_anonymous_verify_batch(pvk._h, n, xts, ptr(bal), ptr(ge), 0, ptr(ok), ptr(refusal)))
            for i in np.nonzero((ok & sig_ok) == 0)[0]:
                for j in range(RING * i, RING * i + RING):
                    add_ops[j].flags |= SKIP
            lib.check(lib.zk_elgamal_ledger_apply(n_acc, ptr(pen_slots), RING * n, add_ops, 0, ptr(pen_out), None, ptr(slot_st), ptr(add_st)))

        def check_sequence():
            assert ok.all() and sig_ok.all() and not refusal.any(), "the block is not honest"
            results["sequence"] = (bal_out.tobytes(), pen_out.tobytes())

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
        row["n_accounts"], row["points_decoded"] = n_acc, stats.points_decoded
        row["sequence_points_decoded"] = (51 * n + 1) + 2 * (n_acc + n_acc) + 2 * (n_acc + RING * n)   # the verifier, then every slot and op point of the two ledger calls
        spread = row["sequence"]["max_ms"] - row["sequence"]["min_ms"]
        row["sequence_spread_ms"] = round(spread, 4)
        row["execute_not_slower_than_sequence_by_more_than_its_spread"] = row["execute"]["median_ms"] <= row["sequence"]["median_ms"] + spread
        out["sizes"][str(n)] = row
        pvk.close()
    line = json.dumps(out)
    print(line)
    if args:
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
