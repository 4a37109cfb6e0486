"""A block's ElGamal balance updates (zk_elgamal_ledger_apply) against a plain sequential model over oracle/jubjub.py: the
reference's loop restated - a dict of slot values, the ops in index order, Ciphertext::add / ::sub (core/primitives/src/
ciphertext.rs:90-100), IntoXY's verdict on every point from xt_verify_cases.expected.  Every function takes `lib` (a ZkLib
over one build of the C ABI), as tests/xt_verify_cases.py does; `device` None = the host form."""
import ctypes as C
import functools

import numpy as np

import zero_chain_amd as zk
from zero_chain_amd import _lib as zl
from oracle import jubjub as jj
import xt_verify_cases as xc

W = zk.LEDGER_SCAN_WIDTH
SUB, SKIP = zk.LEDGER_SUBTRACT, zk.LEDGER_SKIP
IDENTITY = xc.enc_y(1)
IDENTITY_SIGNED = xc.enc_y(1, 1)   # x = 0 with the sign bit set: accepted, as the reference and k_into_xy do
ZERO_CT = IDENTITY + IDENTITY      # Ciphertext::zero()


# ---------------------------------------------------------------------------------------------- the model
def _read(enc):
    """(IntoXY status, point or None) of one encoding"""
    st, xy = xc.expected(bytes(enc))
    return st, None if st else (int.from_bytes(xy[:32], "little"), int.from_bytes(xy[32:], "little"))


def _read_ct(left, right):
    """elgamal::Ciphertext::read: (status byte, (left point, right point) or None) - the first point refused names the status"""
    (sl, pl), (sr, pr) = _read(left), _read(right)
    if sl:
        return 1 | (sl << 6), None
    if sr:
        return 2 | (sr << 6), None
    return 0, (pl, pr)


def _write_ct(ct):
    return bytes(64) if ct is None else jj.write_point(ct[0]) + jj.write_point(ct[1])


def _neg(p):
    return ((-p[0]) % jj.R, p[1])


def model(slots, ops):
    """slots: 64-byte strings; ops: (slot, flags, left, right).  Returns (slots_out, before, slot_status, op_status)."""
    state, slot_status = {}, []
    for s, c in enumerate(slots):
        st, val = _read_ct(c[:32], c[32:])
        slot_status.append(st)
        state[s] = val   # None: the stored value cannot be read - nothing is ever added to it
    before, op_status = [], []
    for slot, flags, left, right in ops:
        st, val = _read_ct(left, right)
        op_status.append(st)
        cur = state[slot]
        before.append(_write_ct(cur))
        if cur is None or st or flags & SKIP:
            continue
        if flags & SUB:
            val = (_neg(val[0]), _neg(val[1]))
        state[slot] = (jj.add(cur[0], val[0]), jj.add(cur[1], val[1]))
    return [_write_ct(state[s]) for s in range(len(slots))], before, slot_status, op_status


# ---------------------------------------------------------------------------------------------- the entry, raw
def raw_apply(lib, slots, ops, device, want_before=True, check=True):
    """The entry through ctypes with every output preset to 0xAA.  Returns (status, slots_out, before, slot_status, op_status)."""
    ns, no = len(slots), len(ops)
    sb = np.frombuffer(b"".join(slots), dtype=np.uint8).copy() if ns else None
    arr = (zl.LedgerOp * max(no, 1))()
    for dst, (slot, flags, left, right) in zip(arr, ops):
        dst.slot, dst.flags = slot, flags
        dst.left[:], dst.right[:] = left, right
    so, bo = np.full(max(ns, 1) * 64, 0xAA, dtype=np.uint8), np.full(max(no, 1) * 64, 0xAA, dtype=np.uint8)
    ss, os_ = np.full(max(ns, 1), 0xAA, dtype=np.uint8), np.full(max(no, 1), 0xAA, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.zk_elgamal_ledger_apply(ns, p(sb) if ns else None, no, arr if no else None, -1 if device is None else device, p(so),
                                     p(bo) if want_before else None, p(ss), p(os_))
    if check:
        lib.check(st)
    # nothing is written past the counts, and before_out is left alone when it was not passed
    assert so[64 * ns:].tobytes() == b"\xaa" * (so.size - 64 * ns) and ss[ns:].tobytes() == b"\xaa" * (ss.size - ns)
    assert os_[no:].tobytes() == b"\xaa" * (os_.size - no)
    assert bo[64 * no:].tobytes() == b"\xaa" * (bo.size - 64 * no)
    sob, bob = so.tobytes(), bo.tobytes()
    return (st, [sob[64 * i:64 * i + 64] for i in range(ns)], [bob[64 * i:64 * i + 64] for i in range(no)],
            [int(v) for v in ss[:ns]], [int(v) for v in os_[:no]])


def check_case(lib, device, slots, ops, without_before=False, want=None):
    want = want or model(slots, ops)
    _, so, bo, ss, os_ = raw_apply(lib, slots, ops, device)
    assert ss == want[2], "slot statuses: %s, expected %s" % (ss, want[2])
    assert os_ == want[3], "op statuses differ at %s" % [i for i in range(len(ops)) if os_[i] != want[3][i]][:8]
    assert bo == want[1], "before_out differs at ops %s of %d" % ([i for i in range(len(ops)) if bo[i] != want[1][i]][:8], len(ops))
    assert so == want[0], "slots_out differs at slots %s of %d" % ([s for s in range(len(slots)) if so[s] != want[0][s]][:8], len(slots))
    if without_before:   # before_out = NULL: the same slots_out
        _, so2, bo2, ss2, os2 = raw_apply(lib, slots, ops, device, want_before=False)
        assert (so2, ss2, os2) == (so, ss, os_)
        assert all(b == b"\xaa" * 64 for b in bo2)


# ---------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def _good():
    return xc.pool()[0]


@functools.lru_cache(maxsize=None)
def _bad_by_kind():
    """one refused encoding of each IntoXY kind: not in the field, not on the curve, not in the prime-order subgroup"""
    bad = xc.pool()[1]
    return tuple(next(e for e in bad if xc.expected(e)[0] == k) for k in (1, 2, 3))


def addend(k):
    """distinct ciphertexts for distinct k: (left, right) of accepted encodings"""
    g = _good()
    assert k < len(g) * len(g)
    return g[k % len(g)], g[(k // len(g) + 3 * k + 1) % len(g)]


def stored(k):
    l, r = addend(1000 + k)
    return l + r


def refused_ct(which, k=0):
    """which 0 .. 5: kind which % 3 in the left (which < 3) or the right point"""
    l, r = addend(2000 + k)
    b = _bad_by_kind()[which % 3]
    return (b, r) if which < 3 else (l, b)


def one_slot(n, first=0):
    """n ops on one slot, additions and subtractions mixed, all addends distinct"""
    return [stored(n)], [(0, SUB if i % 3 == 1 else 0) + addend(first + i) for i in range(n)]


def refusals_at(rot):
    """one slot with W + 3 ops; refused at op 0, at both sides of a 64-lane boundary and of a workgroup boundary, and at the last
    op - the six (kind, side) combinations, rotated by rot"""
    slots, ops = one_slot(W + 3, first=50)
    for k, i in enumerate((0, 63, 64, W - 1, W, W + 2)):
        ops[i] = (0, ops[i][1]) + refused_ct((k + rot) % 6, k)
    return slots, ops


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (slots, ops): the shapes at which each piece can go wrong"""
    out = {}
    out["no_ops_three_slots_one_refused"] = ([stored(0), b"".join(refused_ct(4)), stored(1)], [])
    out["one_slot_one_op"] = one_slot(1)
    for n in (2, 63, 64, 65, W - 1, W, W + 1, 2 * W + 3):   # the carry across wave and workgroup boundaries
        out["one_slot_%d_ops" % n] = one_slot(n)
    # a segment that straddles a workgroup boundary
    out["straddle"] = ([stored(2), stored(3)], [(0, 0) + addend(i) for i in range(W - 2)] + [(1, SUB if i == 2 else 0) + addend(300 + i) for i in range(5)])
    # every op on its own slot, W + 1 of them, given in descending order of slot; every third slot has no op at all
    n_slots = (W + 1) * 3 // 2 + 1
    holders = [s for s in range(n_slots) if s % 3 != 1][:W + 1]
    assert len(holders) == W + 1
    out["own_slots_with_gaps"] = ([stored(s % 40) for s in range(n_slots)], [(s, SUB if s % 5 == 0 else 0) + addend(s) for s in reversed(holders)])
    # the ops of two slots alternate (the second slot's run crosses the workgroup boundary in slot-major order)
    out["interleaved_small"] = ([stored(4), stored(5)], [(i & 1, 0) + addend(i) for i in range(20)])
    out["interleaved_large"] = ([stored(6), stored(7)], [(i & 1, SUB if i % 7 == 3 else 0) + addend(i) for i in range(W + 24)])
    # flags and special values
    a = addend(77)
    out["a_then_minus_a"] = ([ZERO_CT], [(0, 0) + a, (0, SUB) + a])
    out["minus_a_from_a"] = ([a[0] + a[1]], [(0, SUB) + a])
    out["from_zero_mixed"] = ([ZERO_CT, ZERO_CT], [(0, 0) + addend(1), (1, SUB) + addend(2), (0, SUB) + addend(3), (1, 0) + addend(4), (0, 0) + addend(5)])
    out["identity_with_sign_bit"] = ([IDENTITY_SIGNED + IDENTITY, stored(8)], [(0, 0) + addend(9), (1, 0, IDENTITY_SIGNED, IDENTITY_SIGNED), (1, SUB, IDENTITY, IDENTITY_SIGNED)])
    # skip: read and judged, not applied
    slots, ops = one_slot(9, first=20)
    ops[4] = (0, ops[4][1] | SKIP) + ops[4][2:]
    out["one_skipped"] = (slots, ops)
    ops = list(ops)
    ops[0] = (0, SKIP | SUB) + ops[0][2:]
    ops[6] = (0, SKIP) + refused_ct(5)
    ops[8] = (0, SKIP) + ops[8][2:]
    out["skipped_first_last_and_refused"] = (slots, ops)
    slots, ops = one_slot(W + 2, first=30)
    for i in (63, 64, W - 1, W):
        ops[i] = (0, ops[i][1] | SKIP) + ops[i][2:]
    out["skipped_at_boundaries"] = (slots, ops)
    # refusals
    for rot in range(6):
        out["refusals_rot%d" % rot] = refusals_at(rot)
    for which in range(6):   # a refused slot with ops on it, between two good slots
        l, r = refused_ct(which, 9)
        out["refused_slot_%d" % which] = ([stored(9), l + r, stored(10)],
                                          [(0, 0) + addend(1), (1, 0) + addend(2), (2, SUB) + addend(3), (1, SUB) + refused_ct((which + 1) % 6), (1, SKIP) + addend(4),
                                           (0, SUB) + addend(5), (2, 0) + addend(6)])
    return out


WITHOUT_BEFORE = ("no_ops_three_slots_one_refused", "one_slot_one_op", "one_slot_65_ops", "one_slot_%d_ops" % (W + 1), "straddle", "own_slots_with_gaps",
                  "interleaved_large", "refused_slot_2")


@functools.lru_cache(maxsize=None)
def expected_of(name):
    """the model's answer for a case, computed once for the three layers"""
    slots, ops = cases()[name]
    return model(list(slots), list(ops))


def run_case(lib, device, name):
    slots, ops = cases()[name]
    check_case(lib, device, list(slots), list(ops), without_before=name in WITHOUT_BEFORE, want=expected_of(name))


def tails_in_two_passes(lib, device):
    """More workgroups than one pass over their tails holds (W of them): slot 0 runs across the first W workgroups into the
    next pass, slot 1 starts inside that pass and crosses a workgroup boundary again.  The fault this is for - the sum that
    waits between two passes - cannot show below W * W ops, and the sequential model takes seconds there.  So every op of a
    slot carries the SAME ciphertext a: the value op i meets is the slot's plus k a, k = the additions minus the subtractions
    before i, which oracle/jubjub.py's mul gives directly; checked at the places around every boundary and at the end.  (The
    order inside a slot is what the other cases see.)"""
    n0, n1 = W * W + 7, W + 9
    sign0, sign1 = (lambda i: SUB if i % 5 == 2 else 0), (lambda i: SUB if i % 4 == 1 else 0)
    a0, a1 = addend(5), addend(6)
    slots = [stored(11), stored(12)]
    ops = [(0, sign0(i)) + a0 for i in range(n0)] + [(1, sign1(i)) + a1 for i in range(n1)]
    _, so, bo, ss, os_ = raw_apply(lib, slots, ops, device)
    assert ss == [0, 0] and not any(os_)

    def value(slot, a, sign, i):   # of the slot before its op i
        k = sum(-1 if sign(j) else 1 for j in range(i)) % jj.FS_MOD
        (_, init), (_, p) = _read_ct(slot[:32], slot[32:]), _read_ct(*a)
        return _write_ct((jj.add(init[0], jj.mul(p[0], k)), jj.add(init[1], jj.mul(p[1], k))))
    near = lambda n, marks: sorted({i for m in marks for i in (m - 1, m, m + 1) if 0 <= i < n})
    for i in near(n0, (0, 64, W, 2 * W, W * W - W, W * W, n0 - 1)):
        assert bo[i] == value(slots[0], a0, sign0, i), "slot 0, op %d" % i
    for i in near(n1, (0, W - 7, n1 - 1)):   # (slot 1 begins at place W * W + 7: its place W - 7 opens a workgroup)
        assert bo[n0 + i] == value(slots[1], a1, sign1, i), "slot 1, op %d" % i
    assert so == [value(slots[0], a0, sign0, n0), value(slots[1], a1, sign1, n1)]


def nothing_to_do(lib, device):
    """both counts 0: every pointer NULL, no buffer touched"""
    assert lib.zk_elgamal_ledger_apply(0, None, 0, None, -1 if device is None else device, None, None, None, None) == 0
    st, so, bo, ss, os_ = raw_apply(lib, [], [], device)
    assert st == 0 and (so, bo, ss, os_) == ([], [], [], [])


def bad_arguments(lib, device):
    """a slot index out of range, an unknown flag bit, a NULL ops with n_ops > 0: InvalidArgument, nothing written"""
    slots, ops = one_slot(3)
    dev = -1 if device is None else device
    for broken, word in (([ops[0], (1, 0) + addend(1), ops[2]], "op 1"), ([ops[0], ops[1], (0, 4) + addend(1)], "op 2"), ([(7, 0) + addend(1)], "op 0")):
        st, so, bo, ss, os_ = raw_apply(lib, slots, broken, device, check=False)
        assert st == 16 and word in lib.zk_last_error().decode()
        assert so == [b"\xaa" * 64] and ss == [0xAA] and set(os_) == {0xAA} and set(bo) == {b"\xaa" * 64}
    sb = np.frombuffer(slots[0], dtype=np.uint8).copy()
    out = np.full(64 + 64 * 3 + 1 + 3, 0xAA, dtype=np.uint8)
    at = lambda k: C.c_void_p(out.ctypes.data + k)
    assert lib.zk_elgamal_ledger_apply(1, sb.ctypes.data_as(C.c_void_p), 3, None, dev, at(0), at(64), at(256), at(257)) == 16
    assert lib.zk_elgamal_ledger_apply(1, None, 0, None, dev, at(0), at(64), at(256), at(257)) == 16
    assert lib.zk_elgamal_ledger_apply(1, sb.ctypes.data_as(C.c_void_p), 0, None, dev, None, None, at(256), None) == 16
    assert out.tobytes() == b"\xaa" * out.size
    with_mirror = zk.ledger_apply  # the mirror raises what the entry reports
    try:
        with_mirror(slots, [(3, 0) + addend(1)], device=device, lib=lib)
    except zk.ZkError as e:
        assert e.variant == "InvalidArgument"
    else:
        raise AssertionError("slot 3 of 1 was accepted")


def mirror(lib, device):
    """zk.ledger_apply: values, None without want_before, refusals as (field, reason)"""
    slots, ops = cases()["refused_slot_4"]
    want = model(list(slots), list(ops))
    pairs = [(s[:32], s[32:]) for s in slots]
    so, bo, sr, opr = zk.ledger_apply(pairs, list(ops), device=device, lib=lib)
    assert (so, bo) == (want[0], want[1])
    names = lambda v: None if not v else (("left", "right")[(v & 63) - 1], zk.INTO_XY_REASONS[v >> 6])
    assert sr == [names(v) for v in want[2]] and opr == [names(v) for v in want[3]]
    assert sr[1] == ("right", "not on the curve") and opr[3] == ("right", "not in the prime-order subgroup")
    so2, none, _, _ = zk.ledger_apply(list(slots), list(ops), device=device, want_before=False, lib=lib)
    assert so2 == so and none is None


def against_elgamal_add(lib, device):
    """8 random ops on 3 slots: folding zk_elgamal_add over the ops on the same library gives the bytes of slots_out"""
    import random
    rng = random.Random(8)
    slots = [stored(20 + s) for s in range(3)]
    ops = [(rng.randrange(3), rng.choice((0, SUB))) + addend(rng.randrange(1500)) for _ in range(8)]
    assert {o[0] for o in ops} == {0, 1, 2} and {o[1] for o in ops} == {0, SUB}
    _, so, bo, _, _ = raw_apply(lib, slots, ops, device)
    cur = list(slots)
    for i, (s, fl, l, r) in enumerate(ops):
        assert bo[i] == cur[s]
        (nl,), (nr,) = zk.elgamal_add([cur[s][:32]], [cur[s][32:]], [l], [r], subtract=bool(fl & SUB), lib=lib)
        cur[s] = nl + nr
    assert so == cur


def two_transfers_from_one_sender(lib, device):
    """End to end on the small key: two transfers of one sender in a block, the second proof made for the balance after the
    first.  The before_out of the sender's ops, fed as enc_balances to verify_confidential_xts, accepts both; the balance from
    before the block for both rejects the second."""
    P, vkb = xc.small_conf_key()
    pts1, proof1 = xc.good_conf(0)
    bal0 = pts1[6] + pts1[7]

    def sender_ops(p):   # sub_enc_balance: the amount, then the fee, each with the shared randomness (lib.rs:178-205)
        return [(0, SUB, p[2], p[4]), (0, SUB, p[5], p[4])]
    after1 = model([bal0], sender_ops(pts1))[0][0]
    pts2 = list(xc.good_conf(1)[0])
    pts2[6], pts2[7] = after1[:32], after1[32:]
    proof2 = xc.trapdoor_proof(P, xc.inputs_of(pts2))
    ops = sender_ops(pts1) + sender_ops(pts2)
    _, so, bo, ss, os_ = raw_apply(lib, [bal0], ops, device)
    assert ss == [0] and os_ == [0] * 4 and bo[0] == bal0 and bo[2] == after1 and so == model([bal0], ops)[0]
    pvk = zk.prepare_verifying_key(vkb, lib=lib)
    try:
        xts = [xc.conf_xt(list(pts1), proof1), xc.conf_xt(pts2, proof2)]
        for x in xts:   # the xt's own field must not be what decides
            x["enc_balance"] = xc.enc_y(2) + xc.enc_y(2)
        epochs = [pts1[9], pts2[9]]
        ok, ref = zk.verify_confidential_xts(pvk, xts, epochs, enc_balances=[(bo[0][:32], bo[0][32:]), (bo[2][:32], bo[2][32:])])
        assert ok == [True, True] and ref == [None, None]
        ok, ref = zk.verify_confidential_xts(pvk, xts, epochs, enc_balances=[(bal0[:32], bal0[32:])] * 2)
        assert ok == [True, False] and ref == [None, None]
    finally:
        pvk.close()
