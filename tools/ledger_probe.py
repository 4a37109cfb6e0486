#!/usr/bin/env python3
"""What a block's balance updates cost (zk_elgamal_ledger_apply), in the entry's two forms and as the library chooses between
them, beside what a caller had before it - one zk_elgamal_add call per op: ONE JSON line.

  shapes:
    transfer_1               one confidential transfer: 4 slots (balance and pending transfer of sender and recipient), 5 ops
                             (rollover of both, amount and fee off the sender's balance, the amount onto the recipient's pending)
    block_64 / _1024 / _4096 that many transfers; one sender or recipient in eight is an account the block has seen already
                             (no second rollover for it, its ops land on the slots it has)
    exchange_1024            1024 ops on one slot
  per shape, wall ms (host clock around the entry, which ends in a device synchronise; two warm repetitions discarded, median of
  seven with min and max, the three forms taken in turn inside every repetition), with before_out:
    host      ZKAMD_INTO_XY_HOST_MAX huge: decode, walk and encode on the host threads
    device    ZKAMD_INTO_XY_HOST_MAX=0: the decoder, the segmented scan and the encoder on the device
    default   the variable unset
    add_loop  the same ops through zk_elgamal_add, one call each, the slot's bytes carried by the caller (one warm repetition,
              median of three); its final state is compared with the entry's slots_out
The ciphertexts: pairs out of 64 distinct prime-order points.
Usage: python tools/ledger_probe.py [out.json]
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
ENV = "ZKAMD_INTO_XY_HOST_MAX"
SUB = 1


def block_shape(n_transfers, rng):
    """(n_slots, [(slot, flags)]): slots 2 a and 2 a + 1 are the balance and the pending transfer of account a"""
    accounts, ops = 0, []

    def draw():
        nonlocal accounts
        if accounts and rng.randrange(8) == 0:
            return rng.randrange(accounts), False
        accounts += 1
        return accounts - 1, True
    for _ in range(n_transfers):
        (s, s_new), (r, r_new) = draw(), draw()
        if s_new:
            ops.append((2 * s, 0))        # rollover: the pending transfer from before the block onto the balance
        if r_new:
            ops.append((2 * r, 0))
        ops.append((2 * s, SUB))          # sub_enc_balance: the amount, the fee
        ops.append((2 * s, SUB))
        ops.append((2 * r + 1, 0))        # add_pending_transfer
    return 2 * accounts, ops


def main():
    import numpy as np
    import zero_chain_amd as zk
    from zero_chain_amd import _lib as zl
    lib = zk.load_library()
    zk.set_host_threads(HOST_THREADS, lib=lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = random.Random(13)
    points = zk.jubjub_base_mul([rng.randrange(1, FS_MODULUS) for _ in range(DISTINCT)], lib=lib)
    ct = lambda: points[rng.randrange(DISTINCT)] + points[rng.randrange(DISTINCT)]

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

    shapes = [("transfer_1", block_shape(1, rng))] + [("block_%d" % n, block_shape(n, rng)) for n in (64, 1024, 4096)]
    shapes.append(("exchange_1024", (1, [(0, SUB if i % 3 == 0 else 0) for i in range(1024)])))
    out = {"probe": "ledger", "host_threads": HOST_THREADS, "distinct": DISTINCT, "shapes": {}}
    for name, (n_slots, shape) in shapes:
        n_ops = len(shape)
        slots = np.frombuffer(b"".join(ct() for _ in range(n_slots)), dtype=np.uint8).copy()
        ops = (zl.LedgerOp * n_ops)()
        for dst, (slot, flags) in zip(ops, shape):
            c = ct()
            dst.slot, dst.flags = slot, flags
            dst.left[:], dst.right[:] = c[:32], c[32:]
        slots_out, before = np.zeros(64 * n_slots, dtype=np.uint8), np.zeros(64 * n_ops, dtype=np.uint8)
        slot_st, op_st = np.zeros(n_slots, dtype=np.uint8), np.zeros(n_ops, dtype=np.uint8)
        results = {}

        def entry(host_max):
            def run():
                if host_max is None:
                    os.environ.pop(ENV, None)
                else:
                    os.environ[ENV] = host_max
                lib.check(lib.zk_elgamal_ledger_apply(n_slots, ptr(slots), n_ops, ops, 0, ptr(slots_out), ptr(before), ptr(slot_st), ptr(op_st)))
            return run

        def check():
            assert not slot_st.any() and not op_st.any(), "a ciphertext of the block was refused"
            want = results.setdefault("slots_out", slots_out.tobytes())
            assert slots_out.tobytes() == want and before.tobytes() == results.setdefault("before", before.tobytes()), "the forms differ"
            slots_out[:] = 0
            before[:] = 0
        row = timed([("host", entry("1000000000")), ("device", entry("0")), ("default", entry(None))], check)
        os.environ.pop(ENV, None)

        state = slots.copy()
        base = state.ctypes.data
        calls = [(C.c_void_p(base + 64 * o.slot), C.c_void_p(base + 64 * o.slot + 32), C.cast(o.left, C.c_void_p), C.cast(o.right, C.c_void_p),
                  1, o.flags & SUB) for o in ops]

        def add_loop():
            state[:] = slots
            for la, ra, lb, rb, n, sub in calls:   # in place: the entry reads its four points before it writes
                lib.check(lib.zk_elgamal_add(la, ra, lb, rb, n, sub, la, ra))

        def check_loop():
            assert state.tobytes() == results["slots_out"], "the loop of zk_elgamal_add ends in another state"
        row["add_loop"] = timed([("add_loop", add_loop)], check_loop, warm=1, reps=3)["add_loop"]
        row["n_slots"], row["n_ops"], row["points"] = n_slots, n_ops, 2 * (n_slots + n_ops)
        out["shapes"][name] = row
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
