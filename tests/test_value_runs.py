"""Value runs (csrc/value_pairs.h RUN_MAX, ntt.h k_build_scalars, msm_types.h MsmSelSet): a stretch of up to RUN_MAX linked variables
that hold the same value in a proof is ONE term of a multiexp over the sum of their bases.

    z P_1 + ... + z P_l = z (P_1 + ... + P_l)

is an identity of the group, so the proof bytes cannot change; what can go wrong is the bookkeeping - a variable emitted twice
or not at all, a byte that names a base the table does not have, the host's counter and the kernel splitting a run differently.

(a) the rule, over integers: k_build_scalars with the bytes and a cap given at run time (the hook zk_hook_build_scalars_runs) on
    hand-made chains, every base replaced by its discrete logarithm mod r.  The rule is restated here in Python (_model) and the
    kernel's slots and bytes must be exactly what it says; on top of that the sums per query, every variable emitted once, the
    terms per run counted by hand, every slot and byte written, cap 2 = the hook of the pairs word for word, and the host's
    counter (count_merges) = the terms the bytes show saved.
(b) the selection in the sort: one multiexp job of 64 slots for 2 proofs with bytes 0, 2, 3, 4 and absent alternates, against
    the integer sum; the same job without bytes against the old sum.
(c) on the GPU: the case of the runs of 1 ... 9, the selection job, and 4 transfer statements through zk_transfer_prove_batch -
    bytes equal under ZKAMD_MERGE_VALUES unset and = 0 and equal to the oracle's discrete-log proof of one of them.  (The
    emulation runs derived_pairs, the longer bases, the maps and the jobs of prove_chunk in
    test_value_pairs.py::test_emulated_transfer_statement_chunk_form.)
(d) the host logic, on the GPU because binding the transfer key to its circuit takes 0.3 s there and 100 s in emulation: every
    longer base of the transfer key (its toxic waste is the oracle's) is the sum of its members, alt is absent exactly where a
    link behind it is, the bits of the kernel's word agree with alt, and the sections lie in the tables in their order."""
import ctypes as C
import functools

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import synth
import helpers
import test_value_pairs as vp

R = bls.R_MOD
CHAIN_MAX = vp.CHAIN_MAX
QUERIES = ("a", "b2", "l", "b1")            # the order of the q arrays, of the counts and of the bytes of a variable's word
CHAIN_OF = {"a": "a", "b2": "b", "l": "l", "b1": "b"}


def _run_max(lib):
    fn = lib.dll.zk_hook_run_max
    fn.restype = C.c_uint32
    fn.argtypes = []
    return int(fn())


def _build_scalars_runs(lib, n_in, n_aux, counts, links, avail, cap, groups, fold, z, r, s):
    fn = lib.dll.zk_hook_build_scalars_runs
    fn.restype = C.c_int32
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cnt = np.array(counts, dtype=np.uint32)
    lk = np.array(links, dtype=np.int32)
    av = np.array(avail, dtype=np.uint32).astype(np.int32)
    ng = np.array([len(q) for q in groups], dtype=np.uint32)
    ptr, mem = [0], []
    for q in groups:
        for members in q:
            mem += members
            ptr.append(len(mem))
    gr = np.array(ptr + mem, dtype=np.uint32)
    w = zk.scalars_to_bytes(z)
    rb, sb = zk.scalars_to_bytes([r]), zk.scalars_to_bytes([s])
    lay = np.zeros(20, dtype=np.uint32)
    names = ("wstride", "cstride", "w_b2v", "w_pair_a", "w_pair_b2", "aux", "rz", "r", "sz", "s", "rs", "in_tail", "pair_l", "pair_b1",
             "pair_a", "w_one", "w_sum_a", "w_sum_b2", "sum_b1", "sum_a")
    # (the layout is that of the hook of the pairs: asked there, with no output)
    L, _, _ = vp._build_scalars(lib, n_in, n_aux, counts, links, groups, fold, z, r, s)
    wo = np.zeros(L["wstride"] * 32, dtype=np.uint8)
    co = np.zeros(L["cstride"] * 32, dtype=np.uint8)
    sw = np.zeros(counts[0] + counts[1] + 1, dtype=np.uint8)
    sc = np.zeros(counts[2] + counts[3] + (counts[0] if fold else 0) + 1, dtype=np.uint8)
    merges = np.zeros(4, dtype=np.uint64)
    lib.check(fn(n_in, n_aux, cnt.ctypes.data, lk.ctypes.data, av.ctypes.data, cap, ng.ctypes.data, gr.ctypes.data, int(fold), w.ctypes.data,
                 rb.ctypes.data, sb.ctypes.data, wo.ctypes.data, wo.size, co.ctypes.data, co.size, sw.ctypes.data, sc.ctypes.data,
                 merges.ctypes.data, lay.ctypes.data))
    assert dict(zip(names, (int(x) for x in lay))) == L
    return L, zk.bytes_to_scalars(wo.tobytes()), zk.bytes_to_scalars(co.tobytes()), sw[:-1], sc[:-1], [int(x) for x in merges]


class RunCase(vp.RuleCase):
    """vp.RuleCase and: drop[query] = the links (by their second variable) whose pair base the query lacks although both ends
    are dense - a sum that came out as the identity; absent = {(query, j, l)}: longer bases that came out as the identity;
    runs = the (variables, chain sets) of every run, for the counts by hand."""

    def __init__(self, n_aux, chains, live, groups, z, drop, absent, runs):
        super().__init__(n_aux, chains, live, groups, z)
        self.drop, self.absent, self.runs = drop, absent, runs


def _case(name):
    rng = synth.SplitMix64(sum(name.encode()) + 78)
    fw = lambda: rng.field(R - (1 << 65)) + (1 << 64)
    n_aux = 120
    nv = 2 + n_aux
    z = [1, fw()] + [fw() for _ in range(n_aux)]
    every, aux = set(range(nv)), set(range(2, nv))
    live = {"a": set(every), "b1": set(every), "b2": set(every), "l": set(aux)}
    chains = {"a": [], "b": [], "l": []}
    groups = {"a": [], "b1": [], "b2": [], "l": []}
    drop = {qn: set() for qn in QUERIES}
    absent, runs = set(), []

    def run(vars_, value, queries=("a", "b", "l")):
        for v in vars_:
            z[v] = value
        for qn in queries:
            chains[qn].append(list(vars_))
        runs.append((list(vars_), queries))

    if name == "runs_1_to_9":
        at = 2
        for k in range(1, 10):
            run(list(range(at, at + 2 * k, 2)), fw())   # (members two apart, other variables between them)
            at += 2 * k + 1
    elif name == "run_of_40":
        run(list(range(2, 42)), fw())                    # cut behind CHAIN_MAX variables: a run of 32 and one of 8
        run(list(range(50, 90)), fw(), queries=("b",))
    elif name == "zeros_inside":
        run(list(range(2, 13)), fw())
        z[5] = 0                                         # runs 2-3-4 and 6 ... 12
        run([20, 21, 22, 23, 24], 0)                     # a chain of zeros merges nothing
        run([30, 31, 32, 33, 34, 35], fw())
        z[30] = 0
    elif name == "another_chains_value":
        v = fw()
        run([2, 3, 4, 5, 6], v)
        run([10, 11, 12], v)                             # another chain with the same value
        z[30] = v                                        # ... and a variable in no chain
        run([40, 41, 42, 43, 44, 45, 46], fw())
        z[43] = v                                        # the middle of a chain holds the OTHER chains' value: runs of 3 and 3
    elif name == "unusable_links":
        run(list(range(2, 10)), fw())                    # two blocks at cap 4: 2 3 4 5 | 6 7 8 9
        drop["a"] |= {3, 9}                              # the first link inside a block; the last link of a block
        drop["l"] |= {5, 6}                              # the last link of a block; the link across the cut (no term crosses it anyway)
        run(list(range(20, 28)), fw())
        live["a"].discard(22)                            # a member with no term in A at all: both its links go
        run([40, 41, 42, 43], fw(), queries=("b",))
        live["b2"].discard(41)                           # b_g1 has the links, b_g2 does not
        run([50, 51, 52], fw(), queries=("b",))
        drop["b2"].add(52)                               # usable in b_g1, not in b_g2, both ends dense
        run(list(range(60, 68)), fw())
        absent |= {("a", 63, 4), ("a", 67, 4), ("a", 66, 3), ("l", 62, 3), ("b1", 63, 4), ("b1", 62, 3)}   # identity sums: the fallback
    elif name == "members_of_groups":
        run(list(range(2, 10)), fw())                    # members of groups of equal bases at every position of a term
        groups["a"] = [[2, 100], [3, 4, 101], [9, 102]]
        groups["b1"] = [[5, 103], [6, 7, 8, 104]]
        groups["b2"] = [[4, 105], [110, 111]]            # (a group no chain touches ...
        z[111] = (R - z[110]) % R                        # ... whose sum is zero)
        run(list(range(20, 27)), fw())
        drop["a"].add(23)
        groups["a"].append([22, 23, 24, 106])            # a group across the end of a term
    elif name == "one_and_r_minus_one":
        run([2, 3, 4, 5, 6], 1)
        run([10, 11, 12, 13, 14, 15, 16], R - 1)
        run([20, 21, 22], 1, queries=("a",))
    else:
        raise KeyError(name)
    return RunCase(n_aux, chains, live, groups, z, drop, absent, runs)


CASES = ["runs_1_to_9", "run_of_40", "zeros_inside", "another_chains_value", "unusable_links", "members_of_groups", "one_and_r_minus_one"]


def _model(nv, pred, succ, z, has, cap):
    """The rule, restated: term[i] = (the last variable of the term that holds i, its length) for every non-zero variable"""
    term = {}
    for i in range(nv):
        if not z[i]:
            continue
        t, p = 0, pred[i]
        while p >= 0 and t < CHAIN_MAX and z[p] == z[i]:
            t, p = t + 1, pred[p]
        if t % cap:
            continue
        mem, k = [i], succ[i]                      # the block that starts at i
        while len(mem) < cap and k >= 0 and z[k] == z[i]:
            mem.append(k)
            k = succ[k]
        s = 0
        while s < len(mem):                        # the longest term from s whose base the query has, then on behind it
            ln = next((l for l in range(len(mem) - s, 1, -1) if has(l, mem[s + l - 1])), 1)
            for m in mem[s:s + ln]:
                term[m] = (mem[s + ln - 1], ln)
            s += ln
    return term


def _check_rule(lib, name, fold, cap):
    c = _case(name)
    nv, n_in = c.nv, c.n_in
    run_max = _run_max(lib)
    assert 2 <= cap <= run_max
    rng = synth.SplitMix64(4243)
    links, succs, preds = [], {}, {}
    for qn in ("a", "b", "l"):
        pred = [-1] * nv
        for chain in c.chains[qn]:
            for p, j in zip(chain, chain[1:]):
                pred[j] = p
        preds[qn], succs[qn] = vp._finalize(lib, pred)
        links += preds[qn] + succs[qn]
    q, counts = {}, {}
    for qn in QUERIES:
        pred = preds[CHAIN_OF[qn]]
        q[qn], k = [-1] * nv, 0
        for j in range(nv):
            if pred[j] >= 0 and j in c.live[qn] and pred[j] in c.live[qn] and j not in c.drop[qn]:
                q[qn][j] = k
                k += 1
        counts[qn] = k
        links += q[qn]

    def has(qn, l, j):   # the base of the l chain members that end at j: the l - 1 links behind it all have their pair bases
        pred = preds[CHAIN_OF[qn]]
        for _ in range(l - 1):
            if j < 0 or q[qn][j] < 0:
                return False
            j = pred[j]
        return True

    def has_base(qn, l, j):
        return has(qn, l, j) and (qn, j, l) not in c.absent

    avail = [sum(1 << (8 * k + l - 1) for k, qn in enumerate(QUERIES) for l in range(3, run_max + 1) if has_base(qn, l, j)) for j in range(nv)]
    r, s = rng.field(R), rng.field(R)
    cnt = [counts[k] for k in QUERIES]
    grp = [c.groups["a"], c.groups["b2"], c.groups["b1"]]
    L, wit, cv, sw, sc, merges = _build_scalars_runs(lib, n_in, c.n_aux, cnt, links, avail, cap, grp, fold, c.z, r, s)
    if cap == 2:   # the rule of the pairs, word for word, and every byte 0 or 2
        L0, wit0, cv0 = vp._build_scalars(lib, n_in, c.n_aux, cnt, links, grp, fold, c.z, r, s)
        assert (L0, wit0, cv0) == (L, wit, cv)
    dl = {qn: [rng.field(R) for _ in range(nv)] for qn in QUERIES}
    for qn in dl:
        for members in c.groups[qn]:
            for i in members:
                dl[qn][i] = dl[qn][members[0]]
    # (query, scalar vector, slot of variable i, slot of pair k, its bytes, slot of group g, factor on the values)
    views = [("a", wit, lambda i: i, L["w_pair_a"], sw, L["w_sum_a"], 1),
             ("b2", wit, lambda i: L["w_b2v"] + i, L["w_pair_b2"], sw[counts["a"]:], L["w_sum_b2"], 1),
             ("l", cv, lambda i: L["aux"] + i - n_in, L["pair_l"], sc, 0, 1),
             ("b1", cv, lambda i: L["rz"] + i, L["pair_b1"], sc[counts["l"]:], L["sum_b1"], r)]
    if fold:
        views.append(("a", cv, lambda i: L["sz"] + i, L["pair_a"], sc[counts["l"] + counts["b1"]:], L["sum_a"], s))
    untouched = (1 << 256) - 1
    for qn, vec, slot, pair0, sel, group0, factor in views:
        pred, succ = preds[CHAIN_OF[qn]], succs[CHAIN_OF[qn]]
        term = _model(nv, pred, succ, c.z, lambda l, j: l <= cap and has_base(qn, l, j), cap)
        # exactly the slots and bytes the rule says
        for i in range(nv):
            if qn == "l" and i < n_in:
                continue
            own = c.z[i] * factor % R if term.get(i, (i, 1))[1] == 1 else 0
            assert vec[slot(i)] == own, (name, qn, i)
            if q[qn][i] >= 0:
                last, ln = term.get(i, (i, 1))
                emits = last == i and ln >= 2
                assert vec[pair0 + q[qn][i]] == (c.z[i] * factor % R if emits else 0), (name, qn, i)
                assert sel[q[qn][i]] == (ln if emits else 0), (name, qn, i, sel[q[qn][i]])
        for k in range(counts[qn]):   # every pair slot and every byte written
            assert vec[pair0 + k] != untouched and sel[k] != 0xff and (sel[k] == 0 or 2 <= sel[k] <= cap)
        # the sum over the bases, from what the kernel wrote alone: own slots, group slots, pair slots on the sum the byte names
        members_of = {}
        for j in range(nv):
            if q[qn][j] >= 0 and sel[q[qn][j]]:
                mem, k = [], j
                for _ in range(int(sel[q[qn][j]])):
                    mem.append(k)
                    k = pred[k]
                assert all(m >= 0 and m in c.live[qn] for m in mem)
                members_of[j] = mem
        grouped = {i for members in c.groups[qn] for i in members}
        want = sum(c.z[i] * dl[qn][i] for i in c.live[qn]) * factor % R
        got = sum(vec[slot(i)] * dl[qn][i] for i in c.live[qn] - grouped)
        got += sum(vec[group0 + k] * dl[qn][members[0]] for k, members in enumerate(c.groups[qn]))
        got += sum(vec[pair0 + q[qn][j]] * sum(dl[qn][m] for m in mem) for j, mem in members_of.items())
        assert got % R == want, (name, qn)
        # every live variable emitted exactly once
        in_term = {}
        for j, mem in members_of.items():
            for m in mem:
                assert m not in in_term, (name, qn, m)
                in_term[m] = j
        for i in c.live[qn]:
            if i not in grouped:
                assert (vec[slot(i)] != 0) + (i in in_term) == (1 if c.z[i] else 0), (name, qn, i)
        for k, members in enumerate(c.groups[qn]):
            assert vec[group0 + k] == sum(c.z[i] for i in members if i not in in_term) * factor % R, (name, qn, k)
        # the host's counter = the terms the bytes show saved
        saved = sum(int(sel[k]) - 1 for k in range(counts[qn]) if sel[k])
        assert merges[QUERIES.index(qn)] == saved, (name, qn, merges, saved)
        # the terms per run, by hand: an unbroken run of n members is ceil(n / cap) terms
        if not c.drop[qn] and not c.absent and all(len(c.live[x]) >= nv - 2 for x in c.live):
            for vars_, queries in c.runs:
                if CHAIN_OF[qn] not in queries or not c.z[vars_[0]] or any(c.z[v] != c.z[vars_[0]] for v in vars_):
                    continue
                terms = sum(1 for v in vars_ if vec[slot(v)] != 0 or (v in grouped and v not in in_term)) + sum(1 for v in vars_ if v in members_of)
                by_hand = sum(-(-n // cap) for n in ([len(vars_)] if len(vars_) <= CHAIN_MAX else [CHAIN_MAX, len(vars_) - CHAIN_MAX]))
                assert terms == by_hand, (name, qn, vars_, terms, by_hand)
    return c, q, counts, views


# the terms of the A query of every case at cap 4 without the fold, counted by hand (the saved terms: sum of l - 1)
SAVED_A_AT_4 = {
    "runs_1_to_9": 0 + 1 + 2 + 3 + 3 + 4 + 5 + 6 + 6,       # a run of n saves n - ceil(n / 4)
    "run_of_40": 24 + 6,                                      # runs of 32 and 8
    "zeros_inside": 2 + (3 + 2) + (3 + 0),                    # 2-3-4 | 6..9, 10..12 | 31..34, 35 alone
    "another_chains_value": (3 + 0) + 2 + 2 + 2,              # 2..5, 6 alone | 10..12 | 40-41-42 | 44-45-46
    # 2 alone (the first link gone), 3 4 5 | 6 7 8, 9 alone (the last link gone);  20 21, 22 out, 23 alone | 24 25 26 27;
    # 60 61 62, 63 alone (no base of 4) | 64 65, 66 67 (no base of 4 at 67, none of 3 at 66: the longest from 64 is the pair)
    "unusable_links": (0 + 2 + 2 + 0) + (1 + 0 + 0 + 3) + (2 + 0 + 1 + 1),
    "members_of_groups": (3 + 3) + (2 + 0 + 2),               # 2..5 | 6..9;  20 21 22, 23 alone (its link gone) | 24 25 26
    "one_and_r_minus_one": (3 + 0) + (3 + 2) + 2,             # 2..5, 6 alone;  10..13 | 14 15 16;  20 21 22
}


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_rule_over_integers(emu_lib, name, fold):
    for cap in range(2, _run_max(emu_lib) + 1):
        c, q, counts, views = _check_rule(emu_lib, name, fold, cap)
        if cap == 4 and not fold:
            qn, vec, slot, pair0, sel, group0, factor = views[0]
            assert sum(int(sel[k]) - 1 for k in range(counts["a"]) if sel[k]) == SAVED_A_AT_4[name], name


# ----------------------------------------------------------------------------------------------
# (b) the selection in the sort
# ----------------------------------------------------------------------------------------------
N_BASES, N_SLOTS, SEL_FIRST, SEL_N, ALT_W = 80, 64, 40, 24, 2


@functools.lru_cache(maxsize=None)
def _select_job():
    """80 bases k_i G with small k_i; a map of 64 slots onto the first 64 (two mapped out); the slots 40 ... 63 are pair slots
    with alternates for l = 3, 4 among the bases 64 ... 79 (some absent); bytes 0, 2, 3, 4 for 2 proofs, 3 and 4 only where
    the alternate is there, and a byte 0 on a slot whose scalar is 0 as the kernel leaves it"""
    rng = synth.SplitMix64(991)
    dlog = [3 + rng.field(1 << 24) for _ in range(N_BASES)]
    bases = b"".join(bls.g1_uncompressed(bls.G1.to_affine(bls.G1.mul(bls.G1_GEN, k))) for k in dlog)
    mp = list(range(N_SLOTS))
    mp[5] = mp[47] = -1
    alt = [-1] * (SEL_N * ALT_W)
    for k in range(SEL_N):
        if k % 3 != 2:
            alt[k * ALT_W] = 64 + (k % 16)
        if k % 4 != 1:
            alt[k * ALT_W + 1] = 64 + ((k * 7 + 3) % 16)
    scalars, sel = [], []
    for p in range(2):
        sc = [rng.field(R) for _ in range(N_SLOTS)]
        sc[3] = 0
        sc[10] = R - 1
        by = []
        for k in range(SEL_N):
            want = (0, 2, 3, 4)[(k + p) % 4]
            if want >= 3 and alt[k * ALT_W + want - 3] < 0:
                want = 2
            if want == 0:
                sc[SEL_FIRST + k] = 0
            by.append(want)
        scalars.append(sc)
        sel.append(by)
    assert {0, 2, 3, 4} <= set(sel[0]) and {0, 2, 3, 4} <= set(sel[1])
    return dlog, bases, mp, alt, scalars, sel


def _run_select(lib, with_sel):
    dlog, bases, mp, alt, scalars, sel = _select_job()
    fn = lib.dll.zk_hook_msm_select
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    ctx = zk.MultiexpContext(1, bases, window_bits=7, lib=lib)
    try:
        sc = zk.scalars_to_bytes(scalars[0] + scalars[1])
        m = np.array(mp, dtype=np.int32)
        by = np.array(sel[0] + sel[1], dtype=np.uint8)
        al = np.array(alt, dtype=np.int32)
        out = np.zeros(2 * 96, dtype=np.uint8)
        lib.check(fn(ctx._h, 2, N_SLOTS, sc.ctypes.data, m.ctypes.data, by.ctypes.data if with_sel else None, al.ctypes.data if with_sel else None,
                     SEL_FIRST, SEL_N, ALT_W, out.ctypes.data))
    finally:
        ctx.close()
    for p in range(2):
        total = 0
        for i in range(N_SLOTS):
            pos = mp[i]
            k = i - SEL_FIRST
            if with_sel and 0 <= k < SEL_N and sel[p][k] >= 3:
                pos = alt[k * ALT_W + sel[p][k] - 3]
            if pos >= 0:
                total += scalars[p][i] * dlog[pos]
        want = bls.g1_uncompressed(bls.G1.to_affine(bls.G1.mul(bls.G1_GEN, total % R)))
        assert out[96 * p:96 * (p + 1)].tobytes() == want, (p, with_sel)


@pytest.mark.parametrize("with_sel", [True, False])
def test_selection_in_the_sort(emu_lib, with_sel):
    _run_select(emu_lib, with_sel)


# ----------------------------------------------------------------------------------------------
# (c) the GPU
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fold", [0, 1])
def test_gpu_rule_runs_1_to_9(gpu_hooks_lib, fold):
    for cap in range(2, _run_max(gpu_hooks_lib) + 1):
        _check_rule(gpu_hooks_lib, "runs_1_to_9", fold, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("with_sel", [True, False])
def test_gpu_selection_in_the_sort(gpu_hooks_lib, with_sel):
    _run_select(gpu_hooks_lib, with_sel)


@pytest.mark.gpu
def test_gpu_four_transfer_statements(gpu_lib, monkeypatch):
    """4 statements through the chunk form (split launch sets, the fold as its own kernel): the bytes with the runs merged, with
    ZKAMD_MERGE_VALUES=0, and the oracle's discrete-log proof of the first"""
    import sys
    sys.path.insert(0, vp.ROOT)
    import bench
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, want = vp._transfer_wanted()
    seed, amount, fee, balance = bench.statement_params(3)
    ws = list(ws) + [tc.make_witness(seed, amount=amount, fee=fee, balance=balance)]
    rs = list(rs) + [(12345678901234567890123 % R, 98765432109876543210987 % R)]
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_lib)
    try:
        sts = zk.transfer_statements([tc.statement_dict(w) for w in ws])
        on, off = vp._on_and_off(monkeypatch, lambda: [p.write() for p in zk.transfer_prove_batch(mats, params, sts, rs)])
        assert len(on) == 4 and on == off
        assert on[0] == want[0]
    finally:
        mats.close()
        params.close()


def _value_runs(lib, params):
    """zk_hook_value_runs: what ensure_derived bound for the longer runs of the (key, circuit) pair"""
    fn = lib.dll.zk_hook_value_runs
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p] * 7
    info = np.zeros(12, dtype=np.uint32)
    lib.check(fn(params._h, info.ctypes.data, None, None, None, None, None))
    run_max, nv, pa, pb2, pl, pb1, xa, xb2, xl, xb1, n1, n2 = (int(x) for x in info)
    w = run_max - 2
    links = np.zeros(11 * nv, dtype=np.int32)
    alt = np.zeros((pa + pb2 + pl + pb1) * w + 1, dtype=np.int32)
    g1 = np.zeros(n1 * 96 + 1, dtype=np.uint8)
    g2 = np.zeros(n2 * 192 + 1, dtype=np.uint8)
    d = np.zeros(nv * 96, dtype=np.uint8)
    lib.check(fn(params._h, info.ctypes.data, links.ctypes.data, alt.ctypes.data, g1.ctypes.data, g2.ctypes.data, d.ctypes.data))
    return dict(run_max=run_max, nv=nv, counts=[pa, pb2, pl, pb1], xbase=[xa, xb2, xl, xb1], n1=n1, n2=n2, links=links, alt=alt,
                g1=g1.tobytes()[:-1], g2=g2.tobytes()[:-1], d=d.tobytes())


@pytest.mark.gpu
def test_gpu_longer_bases_of_the_transfer_key(gpu_hooks_lib):
    """derived_pairs and ensure_derived on the transfer key, whose toxic waste the oracle knows: B(l, j) is the sum of the l chain
    members that end at j for every query, link and l = 3 ... RUN_MAX (all of them at once: a random combination of the bases
    through the library's one-shot multiexp against the same combination of the discrete logs A_i(tau), B_i(tau) - for the l
    query, whose bases are the D block of the derived set, against the same combination of the D points); alt is absent exactly
    where one of the l - 1 links behind j lacks its pair base; the bits of k_build_scalars' word agree with alt; the sections lie
    in the tables in the order [l | b_g1 | a] and [b_g2]."""
    lib = gpu_hooks_lib
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, _ = vp._transfer_wanted()
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    try:
        zk.transfer_prove_batch(mats, params, zk.transfer_statements([tc.statement_dict(ws[0])]), rs[:1])   # binds the key to the circuit
        v = _value_runs(lib, params)
    finally:
        mats.close()
        params.close()
    nv, W, links = v["nv"], v["run_max"] - 2, v["links"]
    assert nv == r1.n_in + r1.n_aux and v["run_max"] == _run_max(lib)
    xa, xb2, xl, xb1 = v["xbase"]
    alt_at = np.cumsum([0] + [c * W for c in v["counts"]])
    rng = synth.SplitMix64(2020)
    dlog = {"a": P.sc["at"], "b1": P.sc["bt"], "b2": P.sc["bt"]}
    n_longer = {}
    for k, qn in enumerate(QUERIES):
        ci = {"a": 0, "b": 1, "l": 2}[CHAIN_OF[qn]]
        pred = links[2 * ci * nv:(2 * ci + 1) * nv]
        q = links[(6 + k) * nv:(7 + k) * nv]
        alt = v["alt"][alt_at[k]:alt_at[k + 1]]
        assert sorted(int(x) for x in q if x >= 0) == list(range(v["counts"][k]))
        seen, weight, coeff = set(), {}, {}
        for j in range(nv):
            word = (int(links[10 * nv + j]) >> (8 * k)) & 0xff
            if q[j] < 0:
                assert word == 0, (qn, j)
                continue
            members, usable = [j, int(pred[j])], True   # the members of the pair; one more per length while the links hold
            for l in range(3, v["run_max"] + 1):
                usable = usable and q[members[-1]] >= 0
                if usable:
                    members.append(int(pred[members[-1]]))
                x = int(alt[q[j] * W + l - 3])
                assert (x >= 0) == usable, (qn, j, l)                    # (no sum of this key is the identity)
                assert bool(word >> (l - 1) & 1) == (x >= 0), (qn, j, l)
                if x >= 0:
                    assert x not in seen and len(members) == l and min(members) >= 0
                    seen.add(x)
                    coeff[x] = c = rng.field(R)
                    for m in members:
                        weight[m] = (weight.get(m, 0) + c) % R
            assert word & 3 == 0 and word >> v["run_max"] == 0, (qn, j)
        assert seen == set(range(len(seen))) and len(seen) > 2000, (qn, len(seen))
        n_longer[qn] = n = len(seen)
        cs = [coeff[x] for x in range(n)]
        if qn == "b2":
            assert v["n2"] == n
            assert zk.multiexp(2, v["g2"], cs, lib=lib) == helpers.g2_of(sum(w * dlog[qn][m] for m, w in weight.items()))
            continue
        first = {"l": 0, "b1": xb1 - xl, "a": xa - xl}[qn]
        got = zk.multiexp(1, v["g1"][96 * first:96 * (first + n)], cs, lib=lib)
        if qn == "l":
            ms = sorted(weight)
            assert all(m >= r1.n_in and not v["d"][96 * m] & 0x40 for m in ms)
            assert got == zk.multiexp(1, b"".join(v["d"][96 * m:96 * (m + 1)] for m in ms), [weight[m] for m in ms], lib=lib)
        else:
            assert got == helpers.g1_of(sum(w * dlog[qn][m] for m, w in weight.items()))
    # the sections in the tables: [l | b_g1 | a] behind the pair sections of the derived table, [b_g2] behind the pairs of the other
    assert xb1 - xl == n_longer["l"] and xa - xb1 == n_longer["b1"] and v["n1"] - (xa - xl) == n_longer["a"]
