"""Value pairs (csrc/value_pairs.h, prover_binding.h derived_pairs, ntt.h k_build_scalars): two linked variables of a proof that hold
the same value are ONE term of a multiexp over the sum of their two bases.

    z_p P_p + z_j P_j = z_j (P_p + P_j)        whenever z_p = z_j

is an identity of the group, so the proof bytes cannot change; what can go wrong is the bookkeeping - a variable emitted twice
or not at all, a pair's slot left over from another proof, a pair taken in a query that has no base for it.

(a) the rule, over integers: k_build_scalars itself (the emulation build, through the hook zk_hook_build_scalars) on hand-made
    chains and values, with every base replaced by its discrete logarithm mod r: sum slot * base == sum z * P exactly, per
    query, and no variable is emitted twice;
(b) the layout: the pairs' sections lie behind everything the plan had before, and are absent without pairs;
(c) the chains of the transfer circuit: deterministic, at most one predecessor and one successor per variable, and on
    statement 0 of the benchmark they merge what a greedy pairing of equal values merges, within 5 %;
(d) proof bytes with ZKAMD_MERGE_VALUES unset and = 0, equal to each other and to the oracle's: one transfer statement through
    the chunk form of the emulation build; on the GPU transfer and anonymous statements and a non-satisfying witness."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import groth16 as g
from oracle import synth
import helpers

R = bls.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_MAX = 32   # csrc/value_pairs.h


# ----------------------------------------------------------------------------------------------
# (a) the rule over integers
# ----------------------------------------------------------------------------------------------
def _finalize(lib, pred):
    fn = lib.dll.zk_hook_chains_finalize
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    p = np.array(pred, dtype=np.int32)
    s = np.zeros(len(pred), dtype=np.int32)
    lib.check(fn(p.ctypes.data, s.ctypes.data, len(pred)))
    return [int(x) for x in p], [int(x) for x in s]


def _build_scalars(lib, n_in, n_aux, counts, links, groups, fold, z, r, s):
    """groups: the lists of member variables of the groups of equal bases of the (a, b_g2, b_g1) queries"""
    fn = lib.dll.zk_hook_build_scalars
    fn.restype = C.c_int32
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    cnt = np.array(counts, dtype=np.uint32)
    lk = np.array(links, dtype=np.int32)
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
    head = (n_in, n_aux, cnt.ctypes.data, lk.ctypes.data, ng.ctypes.data, gr.ctypes.data, int(fold), w.ctypes.data, rb.ctypes.data, sb.ctypes.data)
    lib.check(fn(*head, None, 0, None, 0, lay.ctypes.data))
    names = ("wstride", "cstride", "w_b2v", "w_pair_a", "w_pair_b2", "aux", "rz", "r", "sz", "s", "rs", "in_tail", "pair_l", "pair_b1",
             "pair_a", "w_one", "w_sum_a", "w_sum_b2", "sum_b1", "sum_a")
    L = dict(zip(names, (int(x) for x in lay)))
    wo = np.zeros(L["wstride"] * 32, dtype=np.uint8)
    co = np.zeros(L["cstride"] * 32, dtype=np.uint8)
    lib.check(fn(*head, wo.ctypes.data, wo.size, co.ctypes.data, co.size, lay.ctypes.data))
    return L, zk.bytes_to_scalars(wo.tobytes()), zk.bytes_to_scalars(co.tobytes())


class RuleCase:
    """nv variables (2 inputs: ONE and one more), chains per query (A, B, L) as lists of variable lists, the variables that are
    dense per query (A, B1, B2; L: every aux), the groups of equal bases per query (A, B1, B2), and the values."""

    def __init__(self, n_aux, chains, live, groups, z):
        self.n_in, self.n_aux, self.nv = 2, n_aux, 2 + n_aux
        self.chains, self.live, self.groups, self.z = chains, live, groups, z


def _rule_case(name):
    rng = synth.SplitMix64(sum(name.encode()) + 77)
    fw = lambda: rng.field(R - (1 << 65)) + (1 << 64)
    n_aux = 120
    nv = 2 + n_aux
    z = [1, fw()] + [fw() for _ in range(n_aux)]
    every = set(range(nv))
    aux = set(range(2, nv))
    live = {"a": set(every), "b1": set(every), "b2": set(every), "l": set(aux)}
    chains = {"a": [], "b": [], "l": []}
    groups = {"a": [], "b1": [], "b2": [], "l": []}

    def run(vars_, value, queries=("a", "b", "l")):
        for v in vars_:
            z[v] = value
        for qn in queries:
            chains[qn].append(list(vars_))

    if name == "runs_1_to_6":
        at = 2
        for k in range(1, 7):
            run(list(range(at, at + 2 * k, 2)), fw())   # (members two apart, other variables between them)
            at += 2 * k + 1
    elif name == "run_of_40":
        run(list(range(2, 42)), fw())                    # cut behind CHAIN_MAX variables: a run of 32 and one of 8
        run(list(range(50, 90)), fw(), queries=("b",))   # ... in one query alone
    elif name == "zeros_inside":
        run([2, 3, 4, 5, 6, 7, 8], fw())
        z[4] = 0                                         # runs 2-3 and 5-6-7-8
        run([10, 11, 12], 0)                             # a chain of zeros merges nothing
        run([20, 21, 22, 23], fw())
        z[20] = 0
    elif name == "equal_to_a_non_partner":
        v = fw()
        run([2, 3, 4], v)
        run([10, 11], v)                                 # another chain with the same value
        z[30] = v                                        # ... and a variable in no chain
        run([40, 41, 42], fw())
        z[41] = v                                        # the middle of a chain equals the OTHER chains' value
    elif name == "dense_in_one_query":
        run([2, 3, 4, 5], fw(), queries=("a", "l"))      # chained in A and L, not dense in B at all
        for v in (2, 3, 4, 5):
            live["b1"].discard(v)
            live["b2"].discard(v)
        run([10, 11, 12], fw(), queries=("a", "b", "l"))
        live["a"].discard(11)                            # a link of the A chains whose end has no term in A
        run([20, 21], fw(), queries=("b",))
        live["b2"].discard(21)                           # b_g1 has the pair, b_g2 does not
    elif name == "partner_in_a_group":
        run([2, 3, 4, 5, 6], fw())                       # members of groups of equal bases pair with their own point
        groups["a"] = [[3, 60], [4, 5, 70]]              # (a second variable and an outsider; a whole pair and an outsider)
        groups["b1"] = [[2, 61]]                         # (a first variable)
        groups["b2"] = [[6, 62], [80, 81]]               # (the odd one out at the end of the run; a group no chain touches)
        z[81] = (R - z[80]) % R                          # ... whose sum is zero
    elif name == "one_and_r_minus_one":
        run([2, 3, 4], 1)
        run([10, 11, 12, 13], R - 1)
        run([20, 21], 1, queries=("a",))
    else:
        raise KeyError(name)
    return RuleCase(n_aux, chains, live, groups, z)


RULE_CASES = ["runs_1_to_6", "run_of_40", "zeros_inside", "equal_to_a_non_partner", "dense_in_one_query", "partner_in_a_group",
              "one_and_r_minus_one"]


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("name", RULE_CASES)
def test_rule_over_integers(emu_lib, name, fold):
    c = _rule_case(name)
    nv, n_in = c.nv, c.n_in
    rng = synth.SplitMix64(4242)
    links, succs, preds = [], {}, {}
    for qn in ("a", "b", "l"):
        pred = [-1] * nv
        for chain in c.chains[qn]:
            for p, j in zip(chain, chain[1:]):
                pred[j] = p
        pred, succ = _finalize(emu_lib, pred)
        assert all(p < j for j, p in enumerate(pred))
        preds[qn], succs[qn] = pred, succ
        links += pred + succ
    if name == "run_of_40":   # the cut: variable 2 + 32 starts a chain of its own
        assert preds["a"][2 + CHAIN_MAX] == -1 and preds["a"][2 + CHAIN_MAX - 1] == 2 + CHAIN_MAX - 2 and preds["a"][2 + CHAIN_MAX + 1] == 2 + CHAIN_MAX
    # a query has the pair of a link when both ends have a term of their own there
    q, counts = {}, {}
    for qn, chain_of in (("a", "a"), ("b2", "b"), ("l", "l"), ("b1", "b")):
        q[qn] = [-1] * nv
        k = 0
        for j in range(nv):
            p = preds[chain_of][j]
            if p >= 0 and j in c.live[qn] and p in c.live[qn]:
                q[qn][j] = k
                k += 1
        counts[qn] = k
        links += q[qn]
    r, s = rng.field(R), rng.field(R)
    L, wit, cv = _build_scalars(emu_lib, n_in, c.n_aux, [counts[k] for k in ("a", "b2", "l", "b1")], links,
                                [c.groups["a"], c.groups["b2"], c.groups["b1"]], fold, c.z, r, s)
    # discrete logs of the bases of every query; the members of a group have one point
    dl = {qn: [rng.field(R) for _ in range(nv)] for qn in ("a", "b1", "b2", "l")}
    for qn in dl:
        for members in c.groups[qn]:
            for i in members:
                dl[qn][i] = dl[qn][members[0]]
    # (query, scalar vector, slot of variable i, slot of pair k, slot of group g, factor on the values)
    views = [("a", wit, lambda i: i, L["w_pair_a"], L["w_sum_a"], 1), ("b2", wit, lambda i: L["w_b2v"] + i, L["w_pair_b2"], L["w_sum_b2"], 1),
             ("l", cv, lambda i: L["aux"] + i - n_in, L["pair_l"], 0, 1), ("b1", cv, lambda i: L["rz"] + i, L["pair_b1"], L["sum_b1"], r)]
    if fold:
        views.append(("a", cv, lambda i: L["sz"] + i, L["pair_a"], L["sum_a"], s))
    for qn, vec, slot, pair0, group0, factor in views:
        chain_of = {"a": "a", "b1": "b", "b2": "b", "l": "l"}[qn]
        pred = preds[chain_of]
        grouped = {i for members in c.groups[qn] for i in members}   # (their own slots are mapped out of the job)
        want = sum(c.z[i] * dl[qn][i] for i in c.live[qn]) * factor % R
        got = sum(vec[slot(i)] * dl[qn][i] for i in c.live[qn] - grouped)
        got += sum(vec[group0 + k] * dl[qn][members[0]] for k, members in enumerate(c.groups[qn]))
        got += sum(vec[pair0 + q[qn][j]] * (dl[qn][j] + dl[qn][pred[j]]) for j in range(nv) if q[qn][j] >= 0)
        assert got % R == want, (name, qn)
        merged = 0
        in_pair = {}
        for i in c.live[qn]:   # emitted exactly once: its own slot (its group's sum), or the pair of one of its two links
            as_second = q[qn][i] >= 0 and vec[pair0 + q[qn][i]] != 0
            sc = succs[chain_of][i]
            as_first = sc >= 0 and q[qn][sc] >= 0 and vec[pair0 + q[qn][sc]] != 0
            in_pair[i] = as_second or as_first
            merged += as_second
            if i in grouped:
                assert as_second + as_first <= 1
                continue
            own = vec[slot(i)] != 0
            assert own + as_second + as_first == (1 if c.z[i] else 0), (name, qn, i)
            if own:
                assert vec[slot(i)] == c.z[i] * factor % R
        for k, members in enumerate(c.groups[qn]):   # a group's sum: the members that are in no pair
            assert vec[group0 + k] == sum(c.z[i] for i in members if not in_pair[i]) * factor % R, (name, qn, k)
        # what the cases are for: the merges the rule finds, counted by hand
        if qn == "a" and not fold:
            expect = {"runs_1_to_6": 0 + 1 + 1 + 2 + 2 + 3, "run_of_40": 16 + 4, "zeros_inside": 1 + 2 + 1, "equal_to_a_non_partner": 1 + 1,
                      "dense_in_one_query": 2 + 0, "partner_in_a_group": 2, "one_and_r_minus_one": 1 + 2 + 1}[name]
            assert merged == expect, (name, merged)
    # the slots nobody may leave unwritten: the kernel wrote every slot of the variables and of the pairs (0xff.. = untouched)
    untouched = (1 << 256) - 1
    for i in range(nv):
        assert wit[i] != untouched and wit[L["w_b2v"] + i] != untouched and cv[L["rz"] + i] != untouched
    for k in range(counts["a"]):
        assert wit[L["w_pair_a"] + k] != untouched
    for k in range(counts["b2"]):
        assert wit[L["w_pair_b2"] + k] != untouched
    for k in range(counts["l"]):
        assert cv[L["pair_l"] + k] != untouched
    for k in range(counts["b1"]):
        assert cv[L["pair_b1"] + k] != untouched


# ----------------------------------------------------------------------------------------------
# (b) the layout
# ----------------------------------------------------------------------------------------------
PLAN_WORDS = 32
PAIR_FIELDS = ("pa", "pb2", "pl", "pb1", "w_end", "w_b2v", "w_pair_a", "w_pair_b2", "pair_l", "pair_b1", "pair_a")


def _plans(lib, np_, n_in, n_aux, n_rows, m, groups, derived, counts):
    old = lib.dll.zk_hook_prove_plan
    old.restype = C.c_int32
    old.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]
    new = lib.dll.zk_hook_prove_plan_pairs
    new.restype = C.c_int32
    new.argtypes = old.argtypes[:9] + [C.c_void_p, C.c_void_p, C.c_size_t]
    a = (C.c_uint64 * PLAN_WORDS)()
    b = (C.c_uint64 * 44)()
    cnt = (C.c_uint32 * 4)(*counts)
    lib.check(old(np_, n_in, n_aux, n_rows, m, *groups, int(derived), a, PLAN_WORDS))
    lib.check(new(np_, n_in, n_aux, n_rows, m, *groups, int(derived), cnt, b, 44))
    return [int(x) for x in a], [int(x) for x in b]


@pytest.mark.parametrize("np_", [1, 200])
def test_layout_sections_behind_the_plan(emu_lib, np_):
    n_in, n_aux, n_rows, m, groups = 23, 19955, 19997, 1 << 15, (1543, 1534, 1534)
    nv = n_in + n_aux
    # without pairs, and on the key's own bases whatever the counts: the plan as it was
    for derived, counts in ((True, (0, 0, 0, 0)), (False, (5, 6, 7, 8))):
        old, new = _plans(emu_lib, np_, n_in, n_aux, n_rows, m, groups, derived, counts)
        assert new[:PLAN_WORDS] == old
        f = dict(zip(PAIR_FIELDS, new[PLAN_WORDS:]))
        assert f["w_end"] == old[21] and not any(f[k] for k in PAIR_FIELDS if k != "w_end")
    counts = (5, 6, 7, 8)   # a, b_g2, l, b_g1
    old, new = _plans(emu_lib, np_, n_in, n_aux, n_rows, m, groups, True, counts)
    f = dict(zip(PAIR_FIELDS, new[PLAN_WORDS:]))
    fold = old[16]
    assert fold == (1 if np_ <= 128 else 0)
    # every word of the old plan but the two strides
    assert [x for i, x in enumerate(new[:PLAN_WORDS]) if i not in (21, 31)] == [x for i, x in enumerate(old) if i not in (21, 31)]
    assert (f["pa"], f["pb2"], f["pl"], f["pb1"]) == counts
    assert f["w_end"] == old[21] == f["w_b2v"]
    assert f["w_pair_a"] == f["w_b2v"] + nv and f["w_pair_b2"] == f["w_pair_a"] + 5 and new[21] == f["w_pair_b2"] + 6
    assert f["pair_l"] == old[31] and f["pair_b1"] == f["pair_l"] + 7
    if fold:
        assert f["pair_a"] == f["pair_b1"] + 8 and new[31] == f["pair_a"] + 5
    else:
        assert f["pair_a"] == 0 and new[31] == f["pair_b1"] + 8


# ----------------------------------------------------------------------------------------------
# (c) the chains of the transfer circuit
# ----------------------------------------------------------------------------------------------
def _chains(lib, circuit=0):
    fn = lib.dll.zk_hook_pair_chains
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    nv = C.c_uint32(0)
    lib.check(fn(circuit, None, 0, C.byref(nv)))
    out = np.zeros(8 * nv.value, dtype=np.int32)
    lib.check(fn(circuit, out.ctypes.data, out.size, C.byref(nv)))
    return nv.value, out


def test_chains_are_deterministic_and_chains(emu_lib):
    nv, c = _chains(emu_lib)
    # a second process derives the same chains
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_value_pairs as t; "
            "from zero_chain_amd._lib import ZkLib; nv, c = t._chains(ZkLib(%r)); print(nv, hashlib.sha256(c.tobytes()).hexdigest())"
            % (ROOT, os.path.join(ROOT, "tests"), emu_lib.path))
    import hashlib
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(nv), hashlib.sha256(c.tobytes()).hexdigest()]
    dense = {"a": c[6 * nv:7 * nv], "b": c[7 * nv:8 * nv], "l": np.array([0] * 23 + [1] * (nv - 23))}
    for k, qn in enumerate(("a", "b", "l")):
        pred, succ = c[2 * k * nv:(2 * k + 1) * nv], c[(2 * k + 1) * nv:(2 * k + 2) * nv]
        linked = [j for j in range(nv) if pred[j] >= 0]
        assert len(linked) > 1000, qn
        assert all(pred[j] < j for j in linked)
        assert len({int(pred[j]) for j in linked}) == len(linked)           # one successor per variable
        assert all(succ[pred[j]] == j for j in linked) and sum(1 for j in range(nv) if succ[j] >= 0) == len(linked)
        assert all(dense[qn][j] and dense[qn][pred[j]] for j in linked)     # links inside the query
        depth = [0] * nv
        for j in linked:
            depth[j] = depth[pred[j]] + 1
        assert max(depth) < CHAIN_MAX


def _full_width(v):
    return v >> 64 != 0 and (R - v) >> 64 != 0


def test_chains_merge_what_a_greedy_pairing_merges(emu_lib):
    """statement 0 of the benchmark: per query, the terms the rule merges along the library's chains against the greedy count
    of the oracle's witness - sum of floor(k / 2) over the groups of k query variables with one full-width value"""
    sys.path.insert(0, ROOT)
    import bench
    from oracle import transfer_circuit as tc
    seed, amount, fee, balance = bench.statement_params(0)
    cs = tc.synthesize(tc.make_witness(seed, amount=amount, fee=fee, balance=balance))
    z = list(cs.inputs) + list(cs.aux)
    nv, c = _chains(emu_lib)
    assert nv == len(z)
    dense = {"a": c[6 * nv:7 * nv], "b": c[7 * nv:8 * nv], "l": [0] * len(cs.inputs) + [1] * len(cs.aux)}
    for k, qn in enumerate(("a", "b", "l")):
        pred = c[2 * k * nv:(2 * k + 1) * nv]
        groups = {}
        for i in range(nv):
            if dense[qn][i] and _full_width(z[i]):
                groups[z[i]] = groups.get(z[i], 0) + 1
        greedy = sum(n // 2 for n in groups.values())
        merged = 0
        for j in range(nv):
            if not z[j] or pred[j] < 0:
                continue
            t, p = 0, pred[j]
            while p >= 0 and t < CHAIN_MAX and z[p] == z[j]:
                t, p = t + 1, pred[p]
            merged += t & 1
        print("query %s: full-width terms %d, greedy pairing merges %d, the chains merge %d" % (qn, sum(groups.values()), greedy, merged))
        assert greedy > 1500
        assert abs(merged - greedy) <= 0.05 * greedy, (qn, merged, greedy)


# ----------------------------------------------------------------------------------------------
# (d) proof bytes: the emulation build, then the GPU
# ----------------------------------------------------------------------------------------------
def test_emulated_transfer_statement_chunk_form(emu_lib, monkeypatch):
    """One transfer statement through the chunk form of the emulation build, ZKAMD_MERGE_VALUES unset and = 0: the bytes equal
    each other and the oracle's discrete-log proof.  This is what runs derived_pairs, the pair sections of the maps, the tables
    with the pair bases and the jobs of prove_chunk without a GPU.  The one slow case of the file: the emulation binds the
    transfer key to the circuit in about 100 s (two transforms of 2^15 points in the exponent) of about 140 s."""
    from oracle import transfer_circuit as tc
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, want = _transfer_wanted()
    params = zk.Parameters.read(pk, checked=False, lib=emu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=emu_lib)
    try:
        sts = zk.transfer_statements([tc.statement_dict(ws[0])])
        on, off = _on_and_off(monkeypatch, lambda: [p.write() for p in zk.transfer_prove_batch(mats, params, sts, rs[:1])])
        vp = params.value_pairs
        assert min(vp["bases"].values()) > 1000 and min(vp["expected_merges"].values()) > 500
        assert on == off
        assert on == want[:1]
    finally:
        mats.close()
        params.close()


def _on_and_off(monkeypatch, prove):
    monkeypatch.delenv("ZKAMD_MERGE_VALUES", raising=False)
    on = prove()
    monkeypatch.setenv("ZKAMD_MERGE_VALUES", "0")
    off = prove()
    monkeypatch.delenv("ZKAMD_MERGE_VALUES", raising=False)
    return on, off


@functools.lru_cache(maxsize=None)
def _transfer_wanted():
    """bench statements 0..2, their (r, s), the oracle's discrete-log proofs"""
    sys.path.insert(0, ROOT)
    import bench
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    E = g.Bls12Engine()
    rng = synth.SplitMix64(1717)
    ws, rs, want = [], [], []
    for i in range(3):
        seed, amount, fee, balance = bench.statement_params(i)
        w = tc.make_witness(seed, amount=amount, fee=fee, balance=balance)
        cs = tc.synthesize(w)
        assert cs.which_is_unsatisfied() is None
        ws.append(w)
        rs.append((rng.field(R), rng.field(R)))
        want.append(helpers.expected_proof_trapdoor(P, g.assign(E, r1, cs.inputs, cs.aux), *rs[-1]))
    return ws, rs, want


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["few", "chunk"])
def test_gpu_transfer_statements(gpu_lib, monkeypatch, form):
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, want = _transfer_wanted()
    if form == "chunk":
        monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
        monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_lib)
    try:
        sts = zk.transfer_statements([tc.statement_dict(w) for w in ws])
        on, off = _on_and_off(monkeypatch, lambda: [p.write() for p in zk.transfer_prove_batch(mats, params, sts, rs)])
        vp = params.value_pairs
        print("transfer key: value pairs", vp)
        assert min(vp["bases"].values()) > 1000 and min(vp["expected_merges"].values()) > 500
        assert on == off
        assert on == want
    finally:
        mats.close()
        params.close()


@pytest.mark.gpu
def test_gpu_transfer_witness_that_fails_a_constraint(gpu_hooks_lib, monkeypatch):
    """the route of the statement entries on a caller's witness (the hook of test_live_rows_h): statement 0 with one aux value
    of a run changed, so a constraint fails and a run is cut in two - against bellman's algorithm on the same key"""
    from oracle import cport
    from oracle import transfer_circuit as tc
    import test_live_rows_h as lr
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, _ = _transfer_wanted()
    cs = tc.synthesize(ws[0])
    z = list(cs.inputs) + list(cs.aux)
    nv, c = _chains(gpu_hooks_lib)
    pred_l = c[4 * nv:5 * nv]
    j = next(j for j in range(nv - 1, 0, -1) if pred_l[j] >= 0 and z[pred_l[j]] == z[j] and z[j])   # the second variable of a merged pair
    z[j] = (z[j] + 1) % R
    E = g.Bls12Engine()
    a = g.assign(E, r1, z[:r1.n_in], z[r1.n_in:])
    assert not g.is_satisfied(E, a)
    want = lr._bellman(cport.Params(pk), a, 1 << 15, *rs[0])
    params = zk.Parameters.read(pk, checked=False, lib=gpu_hooks_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_hooks_lib)
    try:
        on, off = _on_and_off(monkeypatch, lambda: lr._derived(gpu_hooks_lib, mats, params, [z], rs[:1]))
        assert params.value_pairs["bases"]["l"] > 1000
        assert on == off == [want]
    finally:
        mats.close()
        params.close()


@pytest.mark.gpu
def test_gpu_anonymous_statements(gpu_lib, monkeypatch):
    from oracle import anonymous_circuit as ac
    r1, _, P, pk = helpers.anonymous_case(2)   # (the key of tests/test_gpu_parity.py: made once a session)
    ws = [ac.make_witness(300 + s, amount=5 + 7 * s, balance=900 + 31 * s) for s in range(2)]
    rng = synth.SplitMix64(1718)
    rs = [(rng.field(R), rng.field(R)) for _ in ws]
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_lib)
    try:
        sts = zk.anonymous_statements([ac.statement_dict(w) for w in ws])
        on, off = _on_and_off(monkeypatch, lambda: zk.anonymous_prove_batch(mats, params, sts, rs))
        assert min(params.value_pairs["bases"].values()) > 1000
        assert [p.write() for p in on] == [p.write() for p in off]
        pvk = zk.prepare_verifying_key(params)
        try:
            inputs = [list(ac.synthesize(w).inputs[1:]) for w in ws]
            assert zk.verify_proofs(pvk, on, inputs) == [True, True]
            assert zk.verify_proofs(pvk, on, inputs[::-1]) == [False, False]   # (the verifier does look at the inputs)
        finally:
            pvk.close()
    finally:
        mats.close()
        params.close()
