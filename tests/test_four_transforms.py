"""The four-transform form of the prover (prover_binding.h ensure_derived, zkamd.cpp prove_chunk): the H query on the coset-Lagrange basis and
the c part of H folded into the bases of the variables, bound to one (key, circuit) pair.

The statement-to-proof entries take it; zk_prove_batch_witness keeps the six transforms over the key's own bases.  Synthetic
circuits have no statement form, so they reach the new route through the test hook zk_hook_prove_batch_witness_derived
(emulation / hooks builds) and are compared, byte for byte, with zk_prove_batch_witness on the same witness and with the
oracle - bellman's algorithm restated in C (oracle/cport.py), which is defined for an assignment that satisfies nothing as
well, and the trapdoor proof for the satisfying ones."""
import ctypes as C

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import cport
from oracle import groth16 as g
from oracle import params_io, synth
import helpers


def _derived_proofs(lib, mats, params, zs, rs):
    """(proofs, has a derived set, identity bases mapped out) through the hook: the route of the statement-to-proof entries"""
    n = len(rs)
    w = zk.scalars_to_bytes([x for z in zs for x in z])
    rsb = zk.scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(192 * n, dtype=np.uint8)
    info = (C.c_uint32 * 2)()
    fn = lib.dll.zk_hook_prove_batch_witness_derived
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.check(fn(params._h, mats._h, n, w.ctypes.data, 0, rsb.ctypes.data, out.ctypes.data, info))
    ob = out.tobytes()
    return [ob[i * 192:(i + 1) * 192] for i in range(n)], info[0], info[1]


def _bellman(cp, a, r, s):
    return cp.create_proof(helpers.le(a.a), helpers.le(a.b), helpers.le(a.c), helpers.le(a.inputs), helpers.le(a.aux),
                           bytes(a.a_aux_density), bytes(a.b_input_density), bytes(a.b_aux_density), bls.fr_le(r), bls.fr_le(s), 1)


# (name, circuit, log2 of the domain): fewer constraints than the domain has points everywhere, so the zero padding of the rows
# and the dropped top coefficient of h are both in play.  The chain circuits never mention an input in C: the K_i of the inputs
# are the identity and must be mapped out; the random circuit puts inputs (ONE among them) and large coefficients into C.
def _chain(seed, n_in, n_aux, extra):
    c = synth.ChainCircuit(seed, n_in, n_aux, extra_rows=extra)
    return c.r1cs, [c.witness(seed * 10 + i) for i in range(2)]


def _random(seed, n_in, n_aux, n_con):
    r1, inputs, aux = synth.random_r1cs(seed, n_in, n_aux, n_con)
    return r1, [(inputs, aux)]


CIRCUITS = {
    "domain2": lambda: _chain(21, 1, 1, 0) + (1,),        # 1 constraint + 1 input row
    "domain4": lambda: _chain(22, 1, 2, 0) + (2,),        # 2 + 1 rows of 4
    "domain32_chain": lambda: _chain(23, 3, 20, 4) + (5,),   # 24 + 3 rows of 32
    "domain32_inputs_in_c": lambda: _random(24, 3, 12, 20) + (5,),   # 20 + 3 rows of 32
}


def four_transform_parity(lib, name):
    r1, witnesses, log_m = CIRCUITS[name]()
    E = g.Bls12Engine()
    P = g.generate_parameters(E, r1, *helpers.TOXIC, scalars_only=True)
    pk = params_io.write_parameters_from_scalars(P.sc, r1.n_in, threads=4)
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    cp = cport.Params(pk)
    try:
        assert params.info["log_domain"] == log_m
        rng = synth.SplitMix64(77)
        zs, asgs, rs, satisfied = [], [], [], []
        for inputs, aux in witnesses:
            zs.append(list(inputs) + list(aux))
            satisfied.append(True)
        # ... and one assignment with a variable changed so that a constraint fails: h is still bellman's truncated vector
        inputs, aux = witnesses[0]
        broken = list(aux)
        broken[-1] = (broken[-1] + 1) % bls.R_MOD
        zs.append(list(inputs) + broken)
        satisfied.append(False)
        for z in zs:
            asgs.append(g.assign(E, r1, z[:r1.n_in], z[r1.n_in:]))
            rs.append((rng.field(bls.R_MOD), rng.field(bls.R_MOD)))
        assert [g.is_satisfied(E, a) for a in asgs] == satisfied
        old = [p.write() for p in zk.create_proofs_from_witness(mats, params, zs, rs)]   # six transforms, the key's bases
        new, has_set, n_identity = _derived_proofs(lib, mats, params, zs, rs)
        assert has_set == 1
        in_c = {v for _, _, lc in r1.constraints for v, c in lc if c % bls.R_MOD}
        never_in_c = [v for v in range(r1.n_in) if v not in in_c]
        assert n_identity >= len(never_in_c)
        if name != "domain32_inputs_in_c":
            assert never_in_c   # the identity route is taken
        for a, (r, s), x, y, ok in zip(asgs, rs, new, old, satisfied):
            assert x == y
            assert x == _bellman(cp, a, r, s)
            if ok:
                assert x == helpers.expected_proof_trapdoor(P, a, r, s)
        # the key's own route is untouched by the set the key now carries
        assert [p.write() for p in zk.create_proofs_from_witness(mats, params, zs, rs)] == old
    finally:
        mats.close()
        params.close()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_emulated_four_transforms_match_the_six(emu_lib, monkeypatch, name):
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    four_transform_parity(emu_lib, name)


def test_emulated_four_transforms_split_launch_sets(emu_lib, monkeypatch):
    """the chunk form: the A jobs on the key's table beside the C' jobs on the derived one, the fold as its own kernel"""
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    four_transform_parity(emu_lib, "domain32_inputs_in_c")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_gpu_four_transforms_match_the_six(gpu_hooks_lib, name):
    four_transform_parity(gpu_hooks_lib, name)


@pytest.mark.gpu
def test_gpu_transfer_statements_wrong_balance_and_two_lanes(gpu_lib, monkeypatch):
    """Three transfer statements through zk_transfer_prove_batch, the second with a remaining balance that does not add up
    (an unsatisfied constraint), each compared with bellman's algorithm on the oracle's assignment; then 65 statements in two
    jobs through the pipeline, whose two lanes bind to the set the key already carries."""
    from oracle import transfer_circuit as tc
    r1, _, P, pk = helpers.transfer_case(1)
    E = g.Bls12Engine()
    ws = [tc.make_witness(60 + i, amount=7 + i, fee=1, balance=90 + i) for i in range(3)]
    ws[1].remaining_balance += 1
    rs = [(9 + i, 4 + 13 * i) for i in range(3)]
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=gpu_lib)
    cp = cport.Params(pk)
    try:
        sts = [tc.statement_dict(w) for w in ws]
        proofs = [p.write() for p in zk.transfer_prove_batch(mats, params, zk.transfer_statements(sts), rs)]
        for i, (w, (r, s), pf) in enumerate(zip(ws, rs, proofs)):
            cs = tc.synthesize(w)
            assert (cs.which_is_unsatisfied() is None) == (i != 1)
            asg = g.assign(E, r1, cs.inputs, cs.aux)
            assert pf == _bellman(cp, asg, r, s)
            if i != 1:
                assert pf == helpers.expected_proof_trapdoor(P, asg, r, s)
        n = 65
        many = zk.transfer_statements([sts[i % 3] for i in range(n)])
        many_rs = [(100 + i, 200 + 3 * i) for i in range(n)]
        want = [p.write() for p in zk.transfer_prove_batch(mats, params, many, many_rs)]
        for i in (0, 1, 2):   # (the chunk form of the batch against the oracle as well)
            cs = tc.synthesize(ws[i])
            assert want[i] == _bellman(cp, g.assign(E, r1, cs.inputs, cs.aux), *many_rs[i])
        monkeypatch.setenv("ZKAMD_WITNESS", "gpu")   # (the lanes are the GPU-witness form of the pipeline)
        pipe = zk.TransferPipeline(mats, params)
        try:
            pipe.submit(many, many_rs)
            pipe.submit(many, many_rs)
            got = [p.write() for p in pipe.wait()]
            assert got == want + want
        finally:
            pipe.close()
    finally:
        mats.close()
        params.close()
