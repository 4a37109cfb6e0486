"""The scan that can forget (csrc/asset_block_exec.h: k_asset_scan, k_asset_carry, k_asset_encode, k_asset_balance_xy) through
zk_hook_ledger_apply_clear - zk_elgamal_ledger_apply's arguments with the internal flag LEDGER_CLEAR = 4 allowed - on the x86
emulation build and, under -m gpu, on the device.  The expected values come from the sequential model of tests/ledger_cases.py
with one more rule: a CLEAR that is neither skipped nor refused leaves Ciphertext::zero() in the slot, whatever it held, the
unreadable included.  With before_out the hook also holds k_asset_balance_xy to k_asset_encode's bytes for every op."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from zero_chain_amd import _lib as zl
from oracle import jubjub as jj
import ledger_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, SUB, SKIP, CLEAR = lc.W, lc.SUB, lc.SKIP, 4


# ---------------------------------------------------------------------------------------------- the model
def model(slots, ops):
    """ledger_cases.model with the clear rule.  Returns (slots_out, before, slot_status, op_status)."""
    state, slot_status = {}, []
    for s, c in enumerate(slots):
        st, val = lc._read_ct(c[:32], c[32:])
        slot_status.append(st)
        state[s] = val
    before, op_status = [], []
    for slot, flags, left, right in ops:
        st, val = lc._read_ct(left, right)
        op_status.append(st)
        cur = state[slot]
        before.append(lc._write_ct(cur))
        if st or flags & SKIP:
            continue
        if flags & CLEAR:
            state[slot] = (jj.ZERO, jj.ZERO)
            continue
        if cur is None:
            continue
        if flags & SUB:
            val = (lc._neg(val[0]), lc._neg(val[1]))
        state[slot] = (jj.add(cur[0], val[0]), jj.add(cur[1], val[1]))
    return [lc._write_ct(state[s]) for s in range(len(slots))], before, slot_status, op_status


def test_the_model_without_a_clear_is_the_ledger_s():
    for name in ("interleaved_small", "skipped_first_last_and_refused", "refused_slot_3"):
        slots, ops = lc.cases()[name]
        assert model(list(slots), list(ops)) == lc.expected_of(name)


def test_the_flag_is_the_source_s_and_stays_internal():
    src = open(os.path.join(ROOT, "zero-chain_amd", "csrc", "asset_block_exec.h")).read()
    assert int(re.search(r"constexpr uint32_t LEDGER_CLEAR = (\d+);", src).group(1)) == CLEAR
    assert CLEAR & (SUB | SKIP) == 0


# ---------------------------------------------------------------------------------------------- the hook, raw
def raw_apply(lib, slots, ops, device=0, want_before=True):
    """the hook through ctypes with every output preset to 0xAA: (status, slots_out, before, slot_status, op_status)"""
    fn = lib.dll.zk_hook_ledger_apply_clear
    fn.restype = C.c_int32
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(zl.LedgerOp), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ns, no = len(slots), len(ops)
    sb = np.frombuffer(b"".join(slots), dtype=np.uint8).copy()
    arr = (zl.LedgerOp * max(no, 1))()
    for dst, (slot, flags, left, right) in zip(arr, ops):
        dst.slot, dst.flags = slot, flags
        dst.left[:], dst.right[:] = left, right
    so, bo = np.full(ns * 64, 0xAA, dtype=np.uint8), np.full(max(no, 1) * 64, 0xAA, dtype=np.uint8)
    ss, os_ = np.full(ns, 0xAA, dtype=np.uint8), np.full(max(no, 1), 0xAA, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = fn(ns, p(sb), no, arr if no else None, device, p(so), p(bo) if want_before else None, p(ss), p(os_))
    sob, bob = so.tobytes(), bo.tobytes()
    return (st, [sob[64 * i:64 * i + 64] for i in range(ns)], [bob[64 * i:64 * i + 64] for i in range(no)], [int(v) for v in ss], [int(v) for v in os_[:no]])


def check_case(lib, slots, ops, want=None):
    want = want or model(slots, ops)
    st, so, bo, ss, os_ = raw_apply(lib, slots, ops)
    assert st == 0, lib.zk_last_error()
    assert ss == want[2] and os_ == want[3]
    assert bo == want[1], "before_out differs at ops %s of %d" % ([i for i in range(len(ops)) if bo[i] != want[1][i]][:8], len(ops))
    assert so == want[0], "slots_out differs at slots %s" % [s for s in range(len(slots)) if so[s] != want[0][s]][:8]
    st, so2, bo2, _, _ = raw_apply(lib, slots, ops, want_before=False)   # (without before_out: the encoder alone, the same slots)
    assert st == 0 and so2 == so and all(b == b"\xaa" * 64 for b in bo2)


# ---------------------------------------------------------------------------------------------- the cases
def with_flags(ops, marks):
    """ops with the flags of marks {index: flags} in place of their own"""
    return [(o[0], marks[i]) + tuple(o[2:]) if i in marks else o for i, o in enumerate(ops)]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    slots, ops = lc.one_slot(9, first=40)
    for where, i in (("first", 0), ("middle", 4), ("last", 8)):
        out["clear_at_the_%s_op" % where] = (slots, with_flags(ops, {i: CLEAR}))
    out["clear_with_the_subtract_bit"] = (slots, with_flags(ops, {4: CLEAR | SUB}))
    out["clear_is_the_only_op"] = ([lc.stored(3)], [(0, CLEAR) + lc.addend(1)])
    slots, ops = lc.one_slot(W + 5, first=60)
    out["clear_at_lane_w_minus_1"] = (slots, with_flags(ops, {W - 1: CLEAR}))
    out["clear_at_lane_0_of_the_next_workgroup"] = (slots, with_flags(ops, {W: CLEAR}))
    out["clear_around_a_wave_boundary"] = (slots, with_flags(ops, {63: CLEAR, 64: CLEAR | SKIP, 65: CLEAR}))
    out["two_clears_one_workgroup"] = (slots, with_flags(ops, {3: CLEAR, 70: CLEAR}))
    out["two_clears_two_workgroups"] = (slots, with_flags(ops, {3: CLEAR, W + 2: CLEAR}))
    out["skipped_clear_does_not_cut"] = (slots, with_flags(ops, {5: CLEAR | SKIP, W - 1: CLEAR | SKIP, W: CLEAR | SKIP | SUB}))
    slots, ops = lc.one_slot(2 * W + 10, first=90)
    for where, i in (("first", 7), ("middle", W + 7), ("last", 2 * W + 7)):
        out["three_workgroups_clear_in_the_%s" % where] = (slots, with_flags(ops, {i: CLEAR}))
    out["three_workgroups_clear_in_each"] = (slots, with_flags(ops, {W - 1: CLEAR, 2 * W - 1: CLEAR, 2 * W + 9: CLEAR}))
    # refused ops beside a clear, and a clear that is itself refused (it is not live: it must not cut)
    slots, ops = lc.one_slot(12, first=120)
    ops = with_flags(ops, {5: CLEAR, 9: CLEAR})
    ops[4] = (0, 0) + lc.refused_ct(1)
    ops[6] = (0, SUB) + lc.refused_ct(4)
    ops[9] = (0, CLEAR) + lc.refused_ct(2)
    out["refused_ops_beside_a_clear"] = (slots, ops)
    # a clear in the slot before one that starts mid-workgroup must not leak; slot 2 takes the carry across the boundary
    slots = [lc.stored(4), lc.stored(5), lc.stored(6)]
    ops = [(0, 0) + lc.addend(i) for i in range(6)] + [(0, CLEAR) + lc.addend(6)] + [(1, SUB if i % 3 == 0 else 0) + lc.addend(200 + i) for i in range(W - 10)] + \
          [(2, 0) + lc.addend(500 + i) for i in range(8)]
    out["clear_in_the_slot_before"] = (slots, ops)
    # slot 0 fills a workgroup and is cleared at its tail; slot 1 starts at lane 0 of the next
    slots, ops = lc.one_slot(W, first=150)
    out["cut_tail_then_a_new_slot"] = (slots + [lc.stored(7)], with_flags(ops, {W - 1: CLEAR}) + [(1, 0) + lc.addend(700 + i) for i in range(5)])
    # a slot that straddles the boundary, cleared in its first part: the carry it takes is cut
    out["straddle_cleared_before_the_boundary"] = ([lc.stored(8), lc.stored(9)], [(0, 0) + lc.addend(i) for i in range(W - 6)] +
                                                   [(1, CLEAR if i == 2 else 0) + lc.addend(300 + i) for i in range(12)])
    # a cleared slot whose stored value cannot be read: a value again after the clear
    l, r = lc.refused_ct(3, 5)
    out["cleared_unreadable_slot"] = ([lc.stored(10), l + r], [(1, 0) + lc.addend(1), (0, 0) + lc.addend(2), (1, CLEAR) + lc.addend(3), (1, 0) + lc.addend(4),
                                                               (1, SUB) + lc.addend(5), (0, SUB) + lc.addend(6)])
    out["unreadable_slot_cleared_by_its_last_op"] = ([l + r], [(0, 0) + lc.addend(1), (0, CLEAR) + lc.addend(3)])
    # the ops of two slots alternate, each slot with clears, the second across the workgroup boundary in slot-major order
    ops = [(i & 1, SUB if i % 7 == 3 else 0) + lc.addend(i) for i in range(W + 24)]
    out["interleaved_with_clears"] = ([lc.stored(11), lc.stored(12)], with_flags(ops, {40: CLEAR, 41: CLEAR, 2 * (W // 2 - 5) + 1: CLEAR, W + 20: CLEAR}))
    return out


CASES = sorted(cases())


@functools.lru_cache(maxsize=None)
def expected_of(name):
    slots, ops = cases()[name]
    return model(list(slots), list(ops))


def run_case(lib, name):
    slots, ops = cases()[name]
    check_case(lib, list(slots), list(ops), want=expected_of(name))


def test_the_cases_clear_what_they_say():
    """stated without the model: after a live clear at the last op the slot is Ciphertext::zero(), a skipped one changes nothing"""
    assert expected_of("clear_at_the_last_op")[0] == [lc.ZERO_CT]
    assert expected_of("unreadable_slot_cleared_by_its_last_op")[0] == [lc.ZERO_CT] and expected_of("unreadable_slot_cleared_by_its_last_op")[1] == [bytes(64)] * 2
    slots, ops = cases()["skipped_clear_does_not_cut"]
    assert expected_of("skipped_clear_does_not_cut")[0] == lc.model(list(slots), [(o[0], o[1] & ~CLEAR) + tuple(o[2:]) for o in ops])[0]
    assert expected_of("cleared_unreadable_slot")[1][3] == lc.ZERO_CT and expected_of("cleared_unreadable_slot")[1][2] == bytes(64)


def clears_in_two_passes(lib):
    """ledger_cases.tails_in_two_passes with clears: slot 0 runs over W + 3 workgroups - more than one pass over the tails holds -
    and is cleared in the first pass (so the sum that waits between the passes is a cut chain, and two workgroups of the second
    pass take it) and again in the second; slot 1 starts behind it and must see neither.  Every op of a slot carries the same
    ciphertext a, so the value op i meets is [the stored value +] k a with k counted from the last clear."""
    p1, p2 = W * W - W - 3, W * W + 2 * W + 5
    n0, n1 = W * W + 3 * W + 7, W + 9
    sign0, sign1 = (lambda i: SUB if i % 5 == 2 else 0), (lambda i: SUB if i % 4 == 1 else 0)
    a0, a1 = lc.addend(5), lc.addend(6)
    slots = [lc.stored(11), lc.stored(12)]
    ops = [(0, CLEAR if i in (p1, p2) else sign0(i)) + a0 for i in range(n0)] + [(1, sign1(i)) + a1 for i in range(n1)]
    st, so, bo, ss, os_ = raw_apply(lib, slots, ops)
    assert st == 0, lib.zk_last_error()
    assert ss == [0, 0] and not any(os_)

    def value(slot, a, sign, i, clears=()):   # of the slot before its op i
        since = max([c + 1 for c in clears if c < i], default=0)
        k = sum(-1 if sign(j) else 1 for j in range(since, i)) % jj.FS_MOD
        (_, init), (_, p) = lc._read_ct(slot[:32], slot[32:]), lc._read_ct(*a)
        if since:
            init = (jj.ZERO, jj.ZERO)
        return lc._write_ct((jj.add(init[0], jj.mul(p[0], k)), jj.add(init[1], jj.mul(p[1], k))))
    near = lambda n, marks: sorted({i for m in marks for i in (m - 1, m, m + 1) if 0 <= i < n})
    marks = (0, W, p1, W * W - W, W * W, W * W + W, W * W + 2 * W, p2, W * W + 3 * W, n0 - 1)
    for i in near(n0, marks):
        assert bo[i] == value(slots[0], a0, sign0, i, (p1, p2)), "slot 0, op %d" % i
    for i in near(n1, (0, W - 7, n1 - 1)):
        assert bo[n0 + i] == value(slots[1], a1, sign1, i), "slot 1, op %d" % i
    assert so == [value(slots[0], a0, sign0, n0, (p1, p2)), value(slots[1], a1, sign1, n1)]


def bad_arguments(lib):
    slots, ops = lc.one_slot(3)
    for broken, word in (([ops[0], (0, 8) + lc.addend(1)], b"op 1"), ([(5, CLEAR) + lc.addend(1)], b"op 0")):
        st, so, bo, ss, os_ = raw_apply(lib, slots, broken)
        assert st == 16 and word in lib.zk_last_error()
        assert so == [b"\xaa" * 64] and ss == [0xAA] and set(os_) == {0xAA} and set(bo) == {b"\xaa" * 64}


# ---------------------------------------------------------------------------------------------- the kernels' source, emulated
@pytest.mark.parametrize("name", CASES)
def test_clear_under_emulation(emu_lib, name):
    run_case(emu_lib, name)


@pytest.mark.parametrize("name", ["one_slot_%d_ops" % (2 * W + 3), "straddle", "own_slots_with_gaps", "interleaved_large", "skipped_at_boundaries", "refusals_rot2",
                                  "refused_slot_4", "no_ops_three_slots_one_refused"])
def test_no_clear_is_the_ledger_under_emulation(emu_lib, name):
    """without a clear the four kernels give what the ledger's give"""
    slots, ops = lc.cases()[name]
    check_case(emu_lib, list(slots), list(ops), want=lc.expected_of(name))


def test_clears_in_two_passes_under_emulation(emu_lib):
    clears_in_two_passes(emu_lib)


def test_bad_arguments_under_emulation(emu_lib):
    bad_arguments(emu_lib)


def test_the_hook_is_not_in_the_shipped_library():
    dll = C.CDLL(zl.LIB_PATH)
    assert not hasattr(dll, "zk_hook_ledger_apply_clear") and hasattr(dll, "zk_asset_block_execute")
    assert hasattr(C.CDLL(zl.HOOKS_LIB_PATH), "zk_hook_ledger_apply_clear")


def test_the_public_entry_still_refuses_the_bit(emu_lib):
    slots, ops = lc.one_slot(2)
    st = lc.raw_apply(emu_lib, slots, with_flags(ops, {1: CLEAR}), 0, check=False)[0]
    assert st == 16 and b"op 1" in emu_lib.zk_last_error()


# ---------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_clear(gpu_hooks_lib, name):
    run_case(gpu_hooks_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_slot_%d_ops" % (2 * W + 3), "own_slots_with_gaps", "interleaved_large", "refused_slot_4"])
def test_gpu_no_clear_is_the_ledger(gpu_hooks_lib, name):
    slots, ops = lc.cases()[name]
    check_case(gpu_hooks_lib, list(slots), list(ops), want=lc.expected_of(name))


@pytest.mark.gpu
def test_gpu_clears_in_two_passes(gpu_hooks_lib):
    clears_in_two_passes(gpu_hooks_lib)


@pytest.mark.gpu
def test_gpu_bad_arguments(gpu_hooks_lib):
    bad_arguments(gpu_hooks_lib)
