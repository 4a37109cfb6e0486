// Which constraint an assignment breaks: a_j * b_j against c_j for every row j < n_con of a fixed R1CS, per assignment, with
// nothing written but one 16-byte verdict per assignment.  The counterpart of the reference's
// TestConstraintSystem::which_is_unsatisfied / is_satisfied (core/proofs/src/circuit/test.rs:253-272) on the matrices and
// the Montgomery assignment that k_r1cs_eval (ntt.h) reads - no key, no transform, no multiexp.  The per-input rows
// Input(i) * 0 = 0 hold by construction and are not visited.
//
// a_j, b_j, c_j are sums of products of a coefficient < r with a limb vector < 2^256, reduced at every step: canonical
// residues, so a_j * b_j and c_j - both in Montgomery form, a bijection of the residues - are compared limb by limb.
#pragma once
#include "ntt.h"

namespace zkdev {

// the layout of zk_r1cs_verdict (include/zkamd.h)
constexpr uint32_t R1CS_SATISFIED = 0xFFFFFFFFu, R1CS_ONE_IS_NOT_ONE = 1u;
constexpr uint32_t R1CS_V_FIRST = 0, R1CS_V_COUNT = 1, R1CS_V_FLAGS = 2, R1CS_V_WORDS = 4;

// Lanes across proofs (LANE_PER_PROOF): one wave per workgroup, R1CS_CHECK_ROWS consecutive rows per wave.
constexpr uint32_t R1CS_CHECK_ROWS = 32, R1CS_CHECK_WAVE = 64;

// The wave a thread is in.  The emulation build runs every thread as a wave of one lane.
ZK_DI uint32_t wave_lane() {
#ifdef ZK_EMU
    return 0;
#else
    return __lane_id();
#endif
}
ZK_DI uint64_t wave_ballot(bool v) {
#ifdef ZK_EMU
    return v ? 1u : 0u;
#else
    return __ballot(v);
#endif
}

// verdict[p] = (satisfied, 0 rows, z_0 != 1 ?): ONE is an input like any other in the assignment
static __global__ void __launch_bounds__(256)
k_r1cs_check_begin(const uint32_t* __restrict__ z, uint32_t nv, uint32_t np, uint32_t* verdict) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const bool one = ld_fr(z + (size_t)p * nv * 8) == Fr::one();
    *reinterpret_cast<uint4*>(verdict + (size_t)p * R1CS_V_WORDS) = make_uint4(R1CS_SATISFIED, 0u, one ? 0u : R1CS_ONE_IS_NOT_ONE, 0u);
}

// bad |= ZK_BAD_SCALAR when one of `count` Montgomery-form scalars is not < r (a caller's assignment that needs no conversion)
static __global__ void __launch_bounds__(256)
k_fr_flag_noncanonical(const uint32_t* __restrict__ in, size_t count, uint32_t* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (fr_geq_r(ld_fr(in + i * 8))) raise_flag(bad, ZK_BAD_SCALAR);
}

ZK_DI Fr r1cs_row_dot(const R1csMat& m, uint32_t row, const uint32_t* zp) {
    Fr acc = Fr::zero();
    for (uint32_t k = m.row_ptr[row], end = m.row_ptr[row + 1]; k < end; k++)
        acc = add(acc, mul(ld_fr(m.coeff + (size_t)k * 8), ld_fr(zp + (size_t)m.col[k] * 8)));
    return acc;
}
ZK_DI bool r1cs_row_unsatisfied(const R1csMat& ma, const R1csMat& mb, const R1csMat& mc, uint32_t row, const uint32_t* zp) {
    const Fr a = r1cs_row_dot(ma, row, zp), b = r1cs_row_dot(mb, row, zp), c = r1cs_row_dot(mc, row, zp);
    return mul(a, b) != c;
}

// verdict[p].first_bad = the lowest unsatisfied row of assignment p, .n_bad += how many (behind k_r1cs_check_begin).
//   LANE_PER_PROOF = false: one thread per (row, proof), k_r1cs_eval's mapping: blockIdx.x * 256 + threadIdx.x = row,
//     blockIdx.y = proof.  The lanes of a wave hold consecutive rows of one proof, so the wave's ballot gives its lowest
//     unsatisfied row and its count, and the lane of that row issues the wave's one atomicMin and one atomicAdd.  A wave waits
//     for its longest row (1 to 250 and more terms in the built-in circuits).
//   LANE_PER_PROOF = true: a wave (one workgroup of 64) takes R1CS_CHECK_ROWS consecutive rows (blockIdx.x) of 64 proofs
//     (blockIdx.y), lane = proof.  Trip counts, row pointers, columns and coefficients are the same over the wave - loaded once
//     for it, through the scalar unit - and only z is a load per lane (one 32-byte sector, as in the other mapping).  A
//     lane owns its proof's verdict: it keeps the minimum and the count of its rows in registers and issues one atomicMin
//     and one atomicAdd at the end, if any row failed.
template <bool LANE_PER_PROOF>
static __global__ void __launch_bounds__(256)
k_r1cs_check(R1csMat ma, R1csMat mb, R1csMat mc, const uint32_t* __restrict__ z, uint32_t* verdict, uint32_t n_con, uint32_t nv,
             uint32_t np) {
    if (LANE_PER_PROOF) {
        const uint32_t p = blockIdx.y * R1CS_CHECK_WAVE + threadIdx.x;
        if (p >= np) return;
        const uint32_t* zp = z + (size_t)p * nv * 8;
        const uint32_t row0 = blockIdx.x * R1CS_CHECK_ROWS, row1 = row0 + R1CS_CHECK_ROWS < n_con ? row0 + R1CS_CHECK_ROWS : n_con;
        uint32_t first = R1CS_SATISFIED, count = 0;
        for (uint32_t row = row0; row < row1; row++)
            if (r1cs_row_unsatisfied(ma, mb, mc, row, zp)) {
                if (!count) first = row;
                count++;
            }
        if (count) {
            uint32_t* v = verdict + (size_t)p * R1CS_V_WORDS;
            atomicMin(v + R1CS_V_FIRST, first);
            atomicAdd(v + R1CS_V_COUNT, count);
        }
    } else {
        const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
        if (row >= n_con) return;
        const size_t p = blockIdx.y;
        const uint64_t bad = wave_ballot(r1cs_row_unsatisfied(ma, mb, mc, row, z + p * nv * 8));
        if (bad && wave_lane() == (uint32_t)__builtin_ctzll(bad)) {
            uint32_t* v = verdict + p * R1CS_V_WORDS;
            atomicMin(v + R1CS_V_FIRST, row);
            atomicAdd(v + R1CS_V_COUNT, (uint32_t)__builtin_popcountll(bad));
        }
    }
}

}  // namespace zkdev
