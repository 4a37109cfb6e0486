"""The tail of a chunk of proofs on rows of 16 lanes (coop_tail.cpp k_ct_upper: the levels above level 1 of every bucket
reduction of a launch set with more than 128 jobs; k_ct_scale_add: the final fold C = s A + C'), every proof against the
oracle.  The batches carry the edge statements of the fold: s = 0, 1 and r - 1, and an r that puts A at the point at
infinity."""
import pytest

import helpers
from oracle import bls12_381 as bls, cport, groth16
import zero_chain_amd as zk


def _a_at_infinity_r(P, asg):
    """the r for which A = alpha + A(tau) + r delta is the point at infinity"""
    sc, rr = P.sc, bls.R_MOD
    z = asg.inputs + asg.aux
    at = sum(zi * a for zi, a in zip(z, sc["at"])) % rr
    return (-(sc["alpha"] + at)) * pow(sc["delta"], -1, rr) % rr


def _pairs(P, asg, n):
    rr = bls.R_MOD
    edges = [(5, 0), (7, 1), (11, rr - 1), (_a_at_infinity_r(P, asg), 13), (_a_at_infinity_r(P, asg), rr - 1)]
    rest = [((0x9E3779B97F4A7C15 * (i + 1)) % rr, (0xC2B2AE3D27D4EB4F * (i + 7) + (i << 200)) % rr) for i in range(n - len(edges))]
    return edges + rest


def _prove(lib, params, pa, pairs):
    return [p.write() for p in zk.create_proofs([pa] * len(pairs), params, pairs)]


def _expected_proofs(P, asg, pairs):
    """helpers.expected_proof_trapdoor for a whole batch: the discrete logs (a, b, c) of every proof from the toxic waste
    (plain Fr arithmetic), then ONE fixed-base multiplication per group in the C oracle instead of three scalar
    multiplications in Python per proof.  The C oracle answers in uncompressed encodings (a = 0 of the edge proofs: the
    point at infinity), re-encoded here as Proof::write compresses them."""
    E = groth16.Bls12Engine()
    logs = [groth16.create_proof_trapdoor(E, P, asg, r, s) for r, s in pairs]
    n = len(pairs)
    g1 = cport.fixed_base_mul(1, helpers.le([a for a, _, _ in logs] + [c for _, _, c in logs]), 8)
    g2 = cport.fixed_base_mul(2, helpers.le([b for _, b, _ in logs]), 8)
    c1 = lambda i: bls.g1_compressed(bls.g1_from_uncompressed(g1[96 * i:96 * (i + 1)], checked=False))
    c2 = lambda i: bls.g2_compressed(bls.g2_from_uncompressed(g2[192 * i:192 * (i + 1)], checked=False))
    return [c1(i) + c2(i) + c1(n + i) for i in range(n)]


def _rows_vs_oracle(lib, sizes):
    r1, asg, P, pk = helpers.small_case(21, 3, 40, 44)
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    try:
        pa = helpers.to_assignment(zk, asg)
        for n in sizes:
            pairs = _pairs(P, asg, n)
            rows = _prove(lib, params, pa, pairs)
            want = _expected_proofs(P, asg, pairs)
            for i in range(n):
                assert rows[i] == want[i], (n, i)
            assert rows[3][:48] == bytes([0xC0]) + bytes(47)   # A at infinity (compressed, infinity flag)
    finally:
        params.close()


def test_batch_tail_rows_emulation(emu_lib, monkeypatch):
    """ZKAMD_FEW_JOBS=1 and ZKAMD_FOLD_IN_MSM_MAX=0: a batch the emulation can afford takes the chunk form of the tail."""
    monkeypatch.setenv("ZKAMD_FEW_JOBS", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "6")
    _rows_vs_oracle(emu_lib, (6,))


@pytest.mark.gpu
def test_batch_tail_rows_gpu(gpu_lib, monkeypatch):
    """129, 256 and 1024 proofs per chunk: the default form of a chunk (more than 128 jobs per launch set)."""
    monkeypatch.setenv("ZKAMD_BATCH_CHUNK", "1024")
    _rows_vs_oracle(gpu_lib, (129, 256, 1024))
