"""The H part of the four-transform prover on the live rows only (prover_binding.h ensure_derived, zkamd.cpp prove_chunk, ntt.h k_h_live_rows).

A circuit with n_rows = n_con + n_in rows on a domain of m points has m - n_rows rows of zero padding: a_j = b_j = c_j = 0 there
for every assignment.  With w the m-th root, H'_t = H_t (t <= m - 2), H'_(m-1) = 0 (bellman's truncation), a_t the coefficients
of a and

    da_j = sum_t t a_t w^(jt)                       s_j = (da_j b_j + a_j db_j) / m        e_k = a_k b_k - c_k
    Lambda_k = (1/m) sum_t w^-kt H'_t               M_k = -(1/m^2) sum_t t w^-kt H'_t

bellman's sum_t h_t H_t, h the truncated icoset_fft((a b - c) / Z), is

    sum_{j < n_rows} s_j Lambda_j + sum_i z_i (sum_k C_ki M_k) + sum_{k < n_rows} e_k (M_k + Lambda_k / (g^m - 1))

for ANY a, b and c = C z.  The first test checks that over integers (the oracle's transforms, H_t = kappa tau^t for a random
tau); the others send circuits through the route (the hook zk_hook_prove_batch_witness_derived) and compare the proof bytes
with the six-transform route over the key's own bases, with bellman's algorithm (oracle/cport.py) and, where the assignment
satisfies the circuit, with the trapdoor proof.

The circuits: 5 live rows on a domain of 32 (bellman's generator would give such a circuit a domain of 8: the key here is
generated over 32 points, the oracle's generator with the domain's size held, and bellman's algorithm is given the rows padded
to that domain), 31 of 32, 33 of 64, and a random circuit of 23 + 3 rows whose C holds inputs (ONE among them) and full-width
coefficients.  The rows of the inputs are Input(i) * 0 = 0 and cannot fail, so "the last live row" of a broken assignment is
the last constraint."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import cport
from oracle import groth16 as g
from oracle import params_io, synth
import helpers

R = bls.R_MOD


# ----------------------------------------------------------------------------------------------
# the identity over integers
# ----------------------------------------------------------------------------------------------
def _identity_sides(E, m, n_rows, a, b, Cm, z, rng):
    """(bellman's sum_t h_t H_t, the three sums of the identity, s on the whole domain) with H_t = kappa tau^t"""
    r = E.r
    exp = m.bit_length() - 1
    w = g.omega_for(E, exp)
    pad = lambda v: list(v) + [0] * (m - len(v))
    c = [sum(co * z[v] for v, co in row) % r for row in Cm]
    tau, kappa = rng.field(r), rng.field(r)
    H = [kappa * pow(tau, t, r) % r for t in range(m - 1)]
    h = g.h_coefficients(E, pad(a), pad(b), pad(c))
    assert len(h) == m - 1   # (bellman drops the top coefficient)
    lhs = sum(x * y for x, y in zip(h, H)) % r
    Hp = H + [0]
    minv = pow(m, -1, r)
    zinv = pow((pow(E.mult_gen, m, r) - 1) % r, -1, r)
    dot = lambda v: g.fft(E, [t * x % r for t, x in enumerate(g.ifft(E, pad(v), w))], w)
    da, db = dot(a), dot(b)
    A, B = pad(a), pad(b)
    s = [(da[j] * B[j] + A[j] * db[j]) * minv % r for j in range(m)]
    lam = g.ifft(E, Hp, w)
    M = [-x * minv % r for x in g.ifft(E, [t * x % r for t, x in enumerate(Hp)], w)]
    e = [(a[k] * b[k] - c[k]) % r for k in range(n_rows)]
    rhs = sum(s[j] * lam[j] for j in range(n_rows))
    rhs += sum(z[v] * co * M[k] for k, row in enumerate(Cm) for v, co in row)
    rhs += sum(e[k] * (M[k] + lam[k] * zinv) for k in range(n_rows))
    return lhs, rhs % r, s, e


@pytest.mark.parametrize("m,n_rows", [(4, 1), (4, 3), (4, 4), (8, 1), (8, 5), (8, 7), (8, 8), (16, 9), (16, 15), (32, 1), (32, 5),
                                      (32, 31), (32, 32)])
def test_identity_over_integers(m, n_rows):
    E = g.Bls12Engine()
    rng = synth.SplitMix64(1000 * m + n_rows)
    nv = 6
    z = [1] + [rng.field(R) for _ in range(nv - 1)]
    # C: one to three entries per row, full-width and small coefficients, ONE among the variables
    Cm = [[(rng.below(nv), rng.field(R) if rng.below(2) else rng.below(5) + 1) for _ in range(1 + rng.below(3))] for _ in range(n_rows)]
    c = [sum(co * z[v] for v, co in row) % R for row in Cm]
    a = [rng.field(R - 1) + 1 for _ in range(n_rows)]
    b_ok = [c[k] * pow(a[k], -1, R) % R for k in range(n_rows)]
    failing = [[], [0], [n_rows - 1], sorted({0, n_rows // 2, n_rows - 1}), list(range(n_rows))]
    for rows in failing:
        b = list(b_ok)
        for k in rows:
            b[k] = (b[k] + 1 + rng.field(R - 1)) % R
        lhs, rhs, s, e = _identity_sides(E, m, n_rows, a, b, Cm, z, rng)
        assert [k for k in range(n_rows) if e[k]] == rows
        assert not any(s[n_rows:])   # the padding rows carry no H scalar
        assert lhs == rhs


# ----------------------------------------------------------------------------------------------
# circuits
# ----------------------------------------------------------------------------------------------
def _chain(seed, n_in, n_aux):
    """a chain circuit, two witnesses, and the variables to change for (the last constraint; three constraints)"""
    c = synth.ChainCircuit(seed, n_in, n_aux)
    r1 = c.r1cs
    used = {v for la, lb, _ in r1.constraints for v, _ in la + lb}
    leaves = [v for v in range(n_in, n_in + n_aux) if v not in used]   # (each in the C of its own row alone)
    last = n_in + n_aux - 1
    assert last in leaves
    three = leaves[-3:] if len(leaves) >= 3 else list(range(n_in, n_in + n_aux))[-3:]
    return r1, [c.witness(seed * 10 + i) for i in range(2)], [last], three


def _random_two_witnesses(seed, n_in, n_aux, n_con):
    """A random circuit that TWO random assignments satisfy: the two entries of a row of C solve a 2 x 2 system, so they are
    full-width; the second entry's variable is any variable, inputs and ONE included.  Three aux variables occur in one row of
    C each and nowhere else (rows 0, 5 and the last): changing them breaks exactly those rows."""
    rng = synth.SplitMix64(seed)
    nv = n_in + n_aux
    zs = [[1] + [rng.field(R - 1) + 1 for _ in range(nv - 1)] for _ in range(2)]
    leaves = {n_con - 1: nv - 1, 0: nv - 2, 5: nv - 3}
    inner = list(range(nv - 3))
    cons, nxt, in_c = [], n_in, set()
    small = lambda: (rng.below(7) + 1) if rng.below(3) else rng.field(R)
    for j in range(n_con):
        la = [(inner[rng.below(len(inner))], small()) for _ in range(1 + rng.below(3))]
        lb = [(inner[rng.below(len(inner))], small()) for _ in range(1 + rng.below(3))]
        u = leaves.get(j)
        if u is None:
            u, nxt = nxt, n_in + (nxt - n_in + 1) % (n_aux - 3)
        while True:
            v = rng.below(n_in) if j % 3 == 0 else inner[rng.below(len(inner))]
            det = (zs[0][u] * zs[1][v] - zs[0][v] * zs[1][u]) % R
            if v != u and det:
                break
        t = [g.eval_lc(la, z, R) * g.eval_lc(lb, z, R) % R for z in zs]
        di = pow(det, -1, R)
        cu = (t[0] * zs[1][v] - t[1] * zs[0][v]) * di % R
        cv = (zs[0][u] * t[1] - zs[1][u] * t[0]) * di % R
        cons.append((la, lb, [(u, cu), (v, cv)]))
        in_c |= {u, v}
    r1 = g.R1CS(n_in, n_aux, cons)
    assert set(range(n_in, nv)) <= in_c and 0 in in_c
    return r1, [(z[:n_in], z[n_in:]) for z in zs], [nv - 1], [nv - 1, nv - 2, nv - 3]


# name -> (builder, log2 of the key's domain)
CIRCUITS = {
    "rows5_of_32": (lambda: _chain(31, 2, 3), 5),
    "rows31_of_32": (lambda: _chain(32, 3, 28), 5),
    "rows33_of_64": (lambda: _chain(33, 3, 30), 6),
    "random_inputs_in_c": (lambda: _random_two_witnesses(34, 3, 12, 20), 5),
}


def _bellman(cp, a, m, r, s):
    pad = lambda v: helpers.le(list(v) + [0] * (m - len(v)))   # the rows on the key's domain
    return cp.create_proof(pad(a.a), pad(a.b), pad(a.c), helpers.le(a.inputs), helpers.le(a.aux), bytes(a.a_aux_density),
                           bytes(a.b_input_density), bytes(a.b_aux_density), bls.fr_le(r), bls.fr_le(s), 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(r1cs, key bytes, [z] * 4, [(r, s)] * 4, expected proofs): two satisfying assignments, one whose last constraint fails,
    one with three failing constraints; expected = bellman's algorithm on the key's domain, = the trapdoor proof where one exists"""
    build, log_m = CIRCUITS[name]
    r1, witnesses, last, three = build()
    E = g.Bls12Engine()
    n_rows = len(r1.with_input_rows())
    assert n_rows <= 1 << log_m
    natural = g.domain_exp
    g.domain_exp = lambda n: log_m   # (the generator over the key's domain, whatever bellman would have picked for the rows)
    try:
        P = g.generate_parameters(E, r1, *helpers.TOXIC, scalars_only=True)
    finally:
        g.domain_exp = natural
    assert P.sc["m"] == 1 << log_m and len(P.sc["h"]) == (1 << log_m) - 1
    pk = params_io.write_parameters_from_scalars(P.sc, r1.n_in, threads=4)
    zs = [list(i) + list(x) for i, x in witnesses]
    for change in (last, three):
        z = list(zs[0])
        for v in change:
            z[v] = (z[v] + 1) % R
        zs.append(z)
    asgs = [g.assign(E, r1, z[:r1.n_in], z[r1.n_in:]) for z in zs]
    failing = [[k for k in range(n_rows) if (a.a[k] * a.b[k] - a.c[k]) % R] for a in asgs]
    n_con = len(r1.constraints)
    assert failing[0] == [] and failing[1] == [] and failing[2] == [n_con - 1] and len(failing[3]) == 3, failing
    rng = synth.SplitMix64(4713)
    rs = [(rng.field(R), rng.field(R)) for _ in zs]
    cp = cport.Params(pk)
    want = [_bellman(cp, a, 1 << log_m, r, s) for a, (r, s) in zip(asgs, rs)]
    for a, (r, s), w in zip(asgs[:2], rs, want):
        assert w == helpers.expected_proof_trapdoor(P, a, r, s)
    return r1, pk, zs, rs, want


def _derived(lib, mats, params, zs, rs):
    n = len(rs)
    w = zk.scalars_to_bytes([x for z in zs for x in z])
    rsb = zk.scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(192 * n, dtype=np.uint8)
    info = (C.c_uint32 * 2)()
    fn = lib.dll.zk_hook_prove_batch_witness_derived
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.check(fn(params._h, mats._h, n, w.ctypes.data, 0, rsb.ctypes.data, out.ctypes.data, info))
    assert info[0] == 1
    ob = out.tobytes()
    return [ob[i * 192:(i + 1) * 192] for i in range(n)]


def _layout(lib, mats, params):
    info = (C.c_uint32 * 7)()
    fn = lib.dll.zk_hook_derived_layout
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.check(fn(params._h, mats._h, info))
    return list(info)


def live_rows_parity(lib, name, batches):
    r1, pk, zs, rs, want = case(name)
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    try:
        assert params.info["log_domain"] == CIRCUITS[name][1]
        assert _layout(lib, mats, params)[0] == 0   # (no set before the route is taken)
        for pick in batches:
            bz, brs, bwant = [zs[i] for i in pick], [rs[i] for i in pick], [want[i] for i in pick]
            assert _derived(lib, mats, params, bz, brs) == bwant
            assert [p.write() for p in zk.create_proofs_from_witness(mats, params, bz, brs)] == bwant   # six transforms
        n_rows = len(r1.constraints) + r1.n_in
        nv = r1.n_in + r1.n_aux
        has, n_h, n_e, n_var, off_a, off_b1, _ = _layout(lib, mats, params)
        assert has == 1
        assert n_h == n_rows and n_e == n_rows   # the H block and the residual block: the live rows, not the domain
        assert n_var == nv and off_a == 2 * n_rows + nv and off_b1 == off_a + params.info["n_a"] + 2
    finally:
        mats.close()
        params.close()


MODES = {"np1": [[0], [1], [2], [3]], "np3": [[0, 2, 3], [3, 1, 2]], "split": [[0, 1, 2, 3]]}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_emulated_live_rows(emu_lib, monkeypatch, name, mode):
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "5")
    if mode == "split":   # the chunk form: the A jobs as a launch set of their own, the fold as its own kernel
        monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
        monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    live_rows_parity(emu_lib, name, MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_gpu_live_rows(gpu_hooks_lib, monkeypatch, name):
    live_rows_parity(gpu_hooks_lib, name, [[0], [0, 1, 2, 3]])
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    live_rows_parity(gpu_hooks_lib, name, [[3, 2, 1, 0]])
