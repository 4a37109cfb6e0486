"""The tail of a chunk of proofs on rows of 16 lanes (coop_tail.cpp k_ct_upper: the levels above level 1 of every bucket
reduction of a launch set with more than 128 jobs; k_ct_scale_add: the final fold C = s A + C'), against the one-lane
kernels (ZKAMD_COOP_TAIL=0) and the oracle.  The batches carry the edge statements of the fold: s = 0, 1 and r - 1, and an
r that puts A at the point at infinity."""
import pytest

import helpers
from oracle import bls12_381 as bls
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


def _rows_vs_lanes(lib, monkeypatch, sizes, sample):
    r1, asg, P, pk = helpers.small_case(21, 3, 40, 44)
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    try:
        pa = helpers.to_assignment(zk, asg)
        for n in sizes:
            pairs = _pairs(P, asg, n)
            monkeypatch.delenv("ZKAMD_COOP_TAIL", raising=False)
            rows = _prove(lib, params, pa, pairs)
            monkeypatch.setenv("ZKAMD_COOP_TAIL", "0")
            lanes = _prove(lib, params, pa, pairs)
            monkeypatch.delenv("ZKAMD_COOP_TAIL", raising=False)
            assert rows == lanes, n
            for i in list(range(5)) + list(range(5, n, max(1, (n - 5) // sample))):
                assert rows[i] == helpers.expected_proof_trapdoor(P, asg, *pairs[i]), (n, i)
            assert rows[3][:48] == bytes([0xC0]) + bytes(47)   # A at infinity (compressed, infinity flag)
    finally:
        params.close()


def test_batch_tail_rows_emulation(emu_lib, monkeypatch):
    """ZKAMD_FEW_JOBS=1 and ZKAMD_FOLD_IN_MSM_MAX=0: a batch the emulation can afford takes the chunk form of the tail."""
    monkeypatch.setenv("ZKAMD_FEW_JOBS", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    monkeypatch.setenv("ZKAMD_WINDOW_BITS", "6")
    _rows_vs_lanes(emu_lib, monkeypatch, (6,), 1)


@pytest.mark.gpu
def test_batch_tail_rows_gpu(gpu_lib, monkeypatch):
    """129, 256 and 1024 proofs per chunk: the default form of a chunk (more than 128 jobs per launch set)."""
    monkeypatch.setenv("ZKAMD_BATCH_CHUNK", "1024")
    _rows_vs_lanes(gpu_lib, monkeypatch, (129, 256, 1024), 6)
