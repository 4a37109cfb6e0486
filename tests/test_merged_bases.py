"""One term per distinct base in the A and B queries (prover_key.h group_equal_points, prover_binding.h ensure_maps, ntt.h k_build_scalars).

Variables with identical QAP columns have EQUAL points in a key, whatever its toxic waste: z_i P + z_j P = (z_i + z_j) P, so
the multiexps of a proof take such a group as one term under the sum of its scalars.  The groups are found from the points of
each query on its own; ZKAMD_MERGE_BASES=0 gives the maps without them.  Proof bytes cannot change: every case compares the
merged proofs with the unmerged ones, with bellman's algorithm restated in C (oracle/cport.py) - defined for an assignment
that satisfies nothing as well - and, for the satisfying assignments, with the proof from the discrete logs; over the key's
own bases (zk_prove_batch_witness) and over the derived ones (the hook zk_hook_prove_batch_witness_derived)."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import cport
from oracle import groth16 as g
from oracle import params_io, synth
import helpers

R = bls.R_MOD
ONE, PUB, N_IN = 0, 1, 2   # the inputs of the hand-made circuits: ONE and one public value
F = lambda k: N_IN + k      # free aux variable k (aux 0 sits right behind the inputs)


def _circuit(n_free, heads, n_con):
    """Rows `heads` = [(A, B)] over the inputs and the free variables, each defining a new aux variable d_j = A(z) B(z) (its C
    column), then rows d_j = (d_(j-1) + PUB) (k ONE + PUB) up to n_con constraints: they add rows and variables, never an
    equal column."""
    cons = []
    for j in range(n_con):
        la, lb = heads[j] if j < len(heads) else ([(F(n_free + j - 1), 1), (PUB, 1)], [(ONE, j + 2), (PUB, 1)])
        cons.append((la, lb, [(F(n_free + j), 1)]))
    return g.R1CS(N_IN, n_free + n_con, cons)


def _witness(r1, pub, free):
    z = [1, pub] + list(free)
    for la, lb, _ in r1.constraints:
        z.append(g.eval_lc(la, z, R) * g.eval_lc(lb, z, R) % R)
    return z


def _fields(seed, n):
    rng = synth.SplitMix64(seed)
    return [rng.field(R) for _ in range(n)]


WIDE = _fields(9001, 2)   # full-width coefficients


def _lc(vs, c=1):
    return [(F(v), c) for v in vs]


# name -> (r1cs, two satisfying assignments, log2 of the domain, (n_merged_a, n_merged_b))
def _cases():
    out = {}
    # two variables with identical A columns
    out["pair_in_a"] = (_circuit(4, [(_lc([0, 1]), _lc([2])), (_lc([0, 1], 3) + [(PUB, 1)], _lc([3]))], 2),
                        [_fields(1, 4), _fields(2, 4)], 2, (1, 0))
    # ... with identical B columns
    out["pair_in_b"] = (_circuit(4, [(_lc([2]), _lc([0, 1])), (_lc([3]) + [(ONE, 1)], _lc([0, 1], 2))], 4),
                        [_fields(3, 4), _fields(4, 4)], 3, (0, 1))
    # one pair identical in both
    out["pair_in_both"] = (_circuit(3, [(_lc([0, 1]), _lc([0, 1])), (_lc([0, 1, 2]), _lc([0, 1], 7) + [(PUB, 1)])], 8),
                           [_fields(5, 3), _fields(6, 3)], 4, (1, 1))
    # a group of three (in A and in B)
    out["triple"] = (_circuit(4, [(_lc([0, 1, 2]), _lc([3])), (_lc([0, 1, 2], 5), _lc([0, 1, 2]) + [(ONE, 1)])], 18),
                     [_fields(7, 4), _fields(8, 4)], 5, (2, 2))
    # a pair of booleans: the sums are 2 and 1
    out["booleans"] = (_circuit(3, [(_lc([0, 1]), _lc([0, 1]) + [(ONE, 3)]), (_lc([2]), [(PUB, 1)])], 2),
                       [[1, 1] + _fields(9, 1), [0, 1] + _fields(10, 1)], 2, (1, 1))
    # a pair whose values sum to 0 mod r: the group's term vanishes
    zero = lambda seed: (lambda v: [v[0], R - v[0], v[1]])(_fields(seed, 2))
    out["zero_sum"] = (_circuit(3, [(_lc([0, 1]) + [(ONE, 1)], _lc([2])), (_lc([0, 1]), _lc([0, 1]) + [(PUB, 1)])], 4),
                       [zero(11), zero(12)], 3, (1, 1))
    # a pair whose first member is the aux variable behind the inputs, under full-width coefficients
    out["input_adjacent_wide"] = (_circuit(4, [(_lc([0, 1], WIDE[0]), _lc([2])), (_lc([3]), _lc([0, 1], WIDE[1]) + [(PUB, 1)])], 9),
                                  [_fields(13, 4), _fields(14, 4)], 4, (1, 1))
    # no equal columns at all
    chain = synth.ChainCircuit(23, 3, 20, extra_rows=4)
    out["none"] = (chain.r1cs, [chain.witness(230 + i) for i in range(2)], 5, (0, 0))
    # a pair (A), a triple (A and B) and a zero-sum pair (A and B) in one circuit of domain 2^5
    mixed = lambda seed: (lambda v: v[:5] + [v[5], R - v[5], v[6]])(_fields(seed, 7))
    out["mixed32"] = (_circuit(8, [(_lc([0, 1]), _lc([7])), (_lc([2, 3, 4]) + [(ONE, 1)], _lc([2, 3, 4], 2)),
                                   (_lc([5, 6]) + [(PUB, 1)], _lc([5, 6]) + [(ONE, 1)])], 18),
                      [mixed(15), mixed(16)], 5, (4, 3))
    for name, (r1, frees, log_m, merged) in out.items():
        zs = [list(f[0]) + list(f[1]) for f in frees] if name == "none" else [_witness(r1, 5 + 11 * i, f) for i, f in enumerate(frees)]
        out[name] = (r1, zs, log_m, merged)
    return out


CASES = _cases()


def identical_columns(r1):
    """(entries - distinct columns) of the A and of the B query, from the matrices: what a key must merge at least"""
    nv = r1.n_in + r1.n_aux
    cols = [[{} for _ in range(nv)] for _ in range(2)]
    for j, (la, lb, _) in enumerate(r1.with_input_rows()):
        for k, lc in enumerate((la, lb)):
            for v, c in lc:
                cols[k][v][j] = (cols[k][v].get(j, 0) + c) % R
    out = []
    for k in range(2):
        live = [tuple(sorted((j, c) for j, c in col.items() if c)) for col in cols[k]]
        live = [c for c in live if c]
        out.append(len(live) - len(set(live)))
    return tuple(out)


def _bellman(cp, a, r, s):
    return cp.create_proof(helpers.le(a.a), helpers.le(a.b), helpers.le(a.c), helpers.le(a.inputs), helpers.le(a.aux),
                           bytes(a.a_aux_density), bytes(a.b_input_density), bytes(a.b_aux_density), bls.fr_le(r), bls.fr_le(s), 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(r1cs, pk bytes, [z] - two satisfying assignments and one with a failing constraint -, [(r, s)], the proofs bellman's
    algorithm makes of them - the satisfying ones checked against the discrete-log proof here, once)"""
    r1, zs, log_m, merged = CASES[name]
    E = g.Bls12Engine()
    assert identical_columns(r1) == merged
    zs = [list(z) for z in zs]
    broken = list(zs[0])
    broken[-1] = (broken[-1] + 1) % R   # the last row's product no longer is its C
    zs.append(broken)
    P = g.generate_parameters(E, r1, *helpers.TOXIC, scalars_only=True)
    pk = params_io.write_parameters_from_scalars(P.sc, r1.n_in, threads=4)
    assert g.domain_exp(len(r1.with_input_rows())) == log_m
    rng = synth.SplitMix64(4711)
    rs = [(rng.field(R), rng.field(R)) for _ in zs]
    asgs = [g.assign(E, r1, z[:r1.n_in], z[r1.n_in:]) for z in zs]
    assert [g.is_satisfied(E, a) for a in asgs] == [True, True, False]
    cp = cport.Params(pk)
    want = [_bellman(cp, a, r, s) for a, (r, s) in zip(asgs, rs)]
    for a, (r, s), w in zip(asgs[:2], rs, want):
        assert w == helpers.expected_proof_trapdoor(P, a, r, s)
    return r1, pk, zs, rs, want


def _derived(lib, mats, params, zs, rs, montgomery=False):
    """the route of the statement-to-proof entries (four transforms over the derived bases), through the hook"""
    n = len(rs)
    w = zk.scalars_to_bytes([x for z in zs for x in z])
    rsb = zk.scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(192 * n, dtype=np.uint8)
    info = (C.c_uint32 * 2)()
    fn = lib.dll.zk_hook_prove_batch_witness_derived
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.check(fn(params._h, mats._h, n, w.ctypes.data, zk.ZK_FR_MONTGOMERY if montgomery else 0, rsb.ctypes.data, out.ctypes.data, info))
    assert info[0] == 1
    ob = out.tobytes()
    return [ob[i * 192:(i + 1) * 192] for i in range(n)]


def _own(lib, mats, params, zs, rs, montgomery=False):
    return [p.write() for p in zk.create_proofs_from_witness(mats, params, zs, rs, montgomery=montgomery)]


def _batches(mode, zs, rs, want):
    """the calls of one mode as (zs, rs, expected proofs)"""
    if mode == "np1":
        return [([z], [x], [w]) for z, x, w in zip(zs, rs, want)]
    if mode == "np3":
        return [(zs, rs, want)]
    pick = [0, 1, 2, 1, 0]
    return [([zs[i] for i in pick], [rs[i] for i in pick], [want[i] for i in pick])]


def merged_parity(lib, monkeypatch, name, mode, pk=None, want=None, routes=(_own, _derived)):
    r1, pk0, zs, rs, want0 = case(name)
    pk, want = pk or pk0, want or want0
    if mode == "np5":   # the chunk form: the fold as its own kernel, the A jobs as a launch set of their own
        monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
        monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    try:
        for bz, brs, bwant in _batches(mode, zs, rs, want):
            for route in routes:
                monkeypatch.delenv("ZKAMD_MERGE_BASES", raising=False)
                merged = route(lib, mats, params, bz, brs)
                monkeypatch.setenv("ZKAMD_MERGE_BASES", "0")
                plain = route(lib, mats, params, bz, brs)
                assert merged == plain
                assert merged == bwant
        monkeypatch.delenv("ZKAMD_MERGE_BASES", raising=False)
        return params.info, params.merged_bases
    finally:
        mats.close()
        params.close()


@pytest.mark.parametrize("mode", ["np1", "np3", "np5"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_merged_proofs_are_the_unmerged_ones(emu_lib, monkeypatch, name, mode):
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    info, merged = merged_parity(emu_lib, monkeypatch, name, mode)
    na, nb = CASES[name][3]
    assert merged == (na, nb, nb)
    assert (info["n_merged_a"], info["n_merged_b1"], info["n_merged_b2"]) == merged


def test_emulated_montgomery_witness_sums(emu_lib, monkeypatch):
    """the sums of a witness that arrives in Montgomery form (the form the witness generators hand over)"""
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    r1, pk, zs, rs, want = case("mixed32")
    zm = [[bls.fr_to_mont(x) for x in z] for z in zs]
    params = zk.Parameters.read(pk, checked=False, lib=emu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=emu_lib)
    try:
        assert _own(emu_lib, mats, params, zm, rs, montgomery=True) == want
        assert _derived(emu_lib, mats, params, zm, rs, montgomery=True) == want
    finally:
        mats.close()
        params.close()


def _query_offsets(pk):
    """byte offsets of the first entries of (a, b_g1, b_g2) in a parameter file, and their lengths"""
    at = 864
    at += 4 + 96 * struct.unpack(">I", pk[at:at + 4])[0]   # vk.ic
    out = []
    for k, size in enumerate((96, 96, 96, 96, 192)):   # h, l, a, b_g1, b_g2
        n = struct.unpack(">I", pk[at:at + 4])[0]
        if k >= 2:
            out.append((at + 4, n))
        at += 4 + size * n
    assert at == len(pk)
    return out


@pytest.mark.parametrize("mode", ["np1", "np3"])
def test_emulated_b_g1_with_a_duplicate_b_g2_lacks(emu_lib, monkeypatch, mode):
    """A key whose b_g1 query holds an equal pair that its b_g2 query does not have (entry 1 overwritten with entry 0: ONE and
    the public input): each query is grouped on its own points, and the proofs are what bellman's algorithm makes of that key."""
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    r1, pk, zs, rs, _ = case("mixed32")
    (_, _), (b1, n_b1), (_, _) = _query_offsets(pk)
    assert n_b1 >= 2 and pk[b1:b1 + 96] != pk[b1 + 96:b1 + 192]
    bent = pk[:b1 + 96] + pk[b1:b1 + 96] + pk[b1 + 192:]
    E = g.Bls12Engine()
    cp = cport.Params(bent)
    want = [_bellman(cp, g.assign(E, r1, z[:r1.n_in], z[r1.n_in:]), r, s) for z, (r, s) in zip(zs, rs)]
    assert want != case("mixed32")[4]
    # (the derived bases are bound to a consistent key: the key's own route)
    _, merged = merged_parity(emu_lib, monkeypatch, "mixed32", mode, pk=bent, want=want, routes=(_own,))
    na, nb = CASES["mixed32"][3]
    assert merged == (na, nb + 1, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 70])
def test_gpu_merged_proofs_are_the_unmerged_ones(gpu_hooks_lib, monkeypatch, n):
    """the 2^5 circuit with the pair, the triple and the zero-sum pair: a few proofs, and a launch set beyond the split"""
    r1, pk, zs, rs, want = case("mixed32")
    params = zk.Parameters.read(pk, checked=False, lib=gpu_hooks_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_hooks_lib)
    try:
        assert params.merged_bases == (4, 3, 3)
        bz, brs, bwant = [zs[i % 3] for i in range(n)], [rs[i % 3] for i in range(n)], [want[i % 3] for i in range(n)]
        for route in (_own, _derived):
            monkeypatch.delenv("ZKAMD_MERGE_BASES", raising=False)
            merged = route(gpu_hooks_lib, mats, params, bz, brs)
            monkeypatch.setenv("ZKAMD_MERGE_BASES", "0")
            assert merged == route(gpu_hooks_lib, mats, params, bz, brs)
            assert merged == bwant
    finally:
        mats.close()
        params.close()


def chain_fold_in_one_launch_set(lib, monkeypatch, route):
    """The fold as its own kernel behind ONE G1 launch set (all C' jobs, then all A jobs): the combination no default reaches
    - the fold leaves the multiexp beyond 128 proofs, where the G1 jobs are two sets since 64.  The smallest circuit with equal
    points in both queries, a proof alone and three in chunks of two: groups, two chunks, a last chunk of one proof."""
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "100000")
    monkeypatch.setenv("ZKAMD_BATCH_CHUNK", "2")
    r1, pk, zs, rs, want = case("booleans")
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    try:
        assert params.merged_bases == (1, 1, 1)
        assert route(lib, mats, params, zs[:1], rs[:1]) == want[:1]
        assert route(lib, mats, params, zs, rs) == want
    finally:
        mats.close()
        params.close()


@pytest.mark.parametrize("route", [_own, _derived], ids=["key", "derived"])
def test_emulated_chain_fold_in_one_launch_set(emu_lib, monkeypatch, route):
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    chain_fold_in_one_launch_set(emu_lib, monkeypatch, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [_own, _derived], ids=["key", "derived"])
def test_gpu_chain_fold_in_one_launch_set(gpu_hooks_lib, monkeypatch, route):
    chain_fold_in_one_launch_set(gpu_hooks_lib, monkeypatch, route)


@pytest.mark.gpu
def test_gpu_transfer_key_groups_and_a_chunk_of_64(gpu_lib):
    """The transfer key merges at least the identical columns of the circuit's matrices, and a chunk of 64 statements proves
    to the discrete-log proofs of the oracle's assignments."""
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    E = g.Bls12Engine()
    na, nb = identical_columns(r1)
    assert na > 1000 and nb > 1000
    ws = [tc.make_witness(300 + i, amount=3 + i, fee=1, balance=50 + 2 * i) for i in range(64)]
    rng = synth.SplitMix64(64)
    rs = [(rng.field(R), rng.field(R)) for _ in ws]
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_lib)
    try:
        ma, mb1, mb2 = params.merged_bases
        print("transfer key: identical columns", (na, nb), "merged", (ma, mb1, mb2))
        assert ma >= na and mb1 >= nb and mb2 >= nb
        assert (params.info["n_merged_a"], params.info["n_merged_b1"], params.info["n_merged_b2"]) == (ma, mb1, mb2)
        proofs = [p.write() for p in zk.transfer_prove_batch(mats, params, zk.transfer_statements([tc.statement_dict(w) for w in ws]), rs)]
        for i in (0, 63):
            cs = tc.synthesize(ws[i])
            assert cs.which_is_unsatisfied() is None
            assert proofs[i] == helpers.expected_proof_trapdoor(P, g.assign(E, r1, cs.inputs, cs.aux), *rs[i])
    finally:
        mats.close()
        params.close()
