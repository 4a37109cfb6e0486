// The multiexp's types and constants (overview: msm.h): the job descriptor and the pair slots that follow a proof's bytes, the
// register budgets, the sizes the kernels and the plan agree on, the digit set of the recoding.  No kernel: this is all that
// the plan (msm_plan.h), the declaration of the group (msm_group.h) and the prover's host code see of the multiexp.
#pragma once
#include "dev_field.h"

// the build has the generated assembly loops (msm_asm_g1.h, msm_asm_g2.h); the x86 emulation build has neither
#if !defined(ZK_EMU) && !defined(ZK_NO_MADD_ASM)
#define ZK_HAVE_MADD_ASM 1
#define ZK_HAVE_RED_ASM 1
#endif

namespace zkdev {

struct MsmJob {
    const uint32_t* scalars;  // n x 8 u32, plain (non-Montgomery) little-endian, each < r
    const int32_t* map;       // n entries: position in the slice-0 table, or -1 (skip);
                              // nullptr = identity
    uint32_t n;               // number of scalars
    uint32_t table_base;      // index of [k = 0][0] of this job's bases inside the group table
    uint32_t n_table;         // table entries per slice
    uint32_t pair_base;       // first slot of this job in the rank / pair arrays
    uint32_t vb_digit;        // 0: width-c NAF over the doubling table (every digit of every scalar);
                              // k + 1: VARIABLE-BASE mode, this job takes digit k of every scalar (see msm_digits)
    uint32_t n_digits;        // variable-base mode: digit positions per scalar
};

// Value runs (ntt.h k_build_scalars): which base a pair slot of a job takes this proof.  A launch set has up to two RANGES of
// jobs with such slots (the C' jobs and the A jobs of one set); the jobs themselves stay as they are.  In job job0 + p, p <
// n_jobs, slot first + k, k < n, is a pair slot whose byte sel[p * stride + k] names the length l of the term it holds this
// proof: l >= 3 takes the base alt[k * alt_w + (l - 3)] in place of map[slot] (static: positions like map's, -1 where the
// table has no such base).  k_build_scalars writes a length only where its word for the variable has the bit, and the bits
// and alt are made in one loop (zkamd.cpp derived_pairs; tests/test_value_runs.py holds the two against each other), so a
// byte that names no base does not occur; if it did, the slot is skipped in both passes of the sort alike - never a read
// outside alt or the table.  All zero: a set without them.
struct MsmSelRange {
    const uint8_t* sel;
    const int32_t* alt;
    uint32_t job0, n_jobs, stride, first, n, alt_w;
};
struct MsmSelSet {
    MsmSelRange r[2];
};

// where the base of scalar i of job j of a set lies in the slice-0 table, or -1 (skip)
ZK_DI int32_t msm_job_pos(const MsmJob& job, const MsmSelSet& S, uint32_t j, uint32_t i) {
    if (!job.map) return (int32_t)i;
    int32_t pos = job.map[i];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const MsmSelRange& r = S.r[h];
        const uint32_t p = j - r.job0, k = i - r.first;
        if (r.sel && p < r.n_jobs && k < r.n) {
            const uint32_t l = r.sel[(size_t)p * r.stride + k];
            if (l >= 3u) pos = l - 3u < r.alt_w ? r.alt[(size_t)k * r.alt_w + (l - 3u)] : -1;
        }
    }
    return pos;
}

// Register budgets.  hipcc sizes a kernel's VGPR allocation from its launch bounds alone (it will
// happily take 256 registers and one wave per SIMD); the second __launch_bounds__ argument (minimum
// waves per SIMD) pins the occupancy the dependent carry chains of the Montgomery product need.
template <class F> struct MsmOcc;
#ifndef ZK_OCC_G1_ACC
#define ZK_OCC_G1_ACC 2
#endif
#ifndef ZK_OCC_G1_RED
#define ZK_OCC_G1_RED 3
#endif
#ifndef ZK_OCC_G2_ACC
#define ZK_OCC_G2_ACC 2
#endif
#ifndef ZK_OCC_G2_RED
#define ZK_OCC_G2_RED 2
#endif
// `tail`: the normalisation kernels (k_xyzz_normalize_export*, setup.h) are chains of dependent field
// operations run by one wave per SIMD at most - occupancy buys nothing there, spilled registers cost
// latency - so they take the whole register file.
#ifndef ZK_OCC_G1_TAIL
#define ZK_OCC_G1_TAIL 2
#endif
#ifndef ZK_OCC_G2_TAIL
#define ZK_OCC_G2_TAIL 1
#endif
template <> struct MsmOcc<Fq> { static constexpr int acc = ZK_OCC_G1_ACC, red = ZK_OCC_G1_RED, tail = ZK_OCC_G1_TAIL; };
template <> struct MsmOcc<Fq2> { static constexpr int acc = ZK_OCC_G2_ACC, red = ZK_OCC_G2_RED, tail = ZK_OCC_G2_TAIL; };
template <> struct MsmOcc<Fq2x> { static constexpr int acc = ZK_OCC_G2_ACC, red = ZK_OCC_G2_RED, tail = ZK_OCC_G2_TAIL; };

// Longest run of points one accumulation thread walks (`seg`, a launch parameter): 256 when
// thousands of jobs fill the machine (fewer task partials to merge in the reduction), 64 for a
// single job (more, shorter tasks to spread over the CUs).  MSM_SEG_MAX sizes the class arrays.
constexpr uint32_t MSM_SEG_MAX = 256;
constexpr uint32_t MSM_NPOS = 255;  // table slices: 2^k * P for k = 0 .. 254
// buckets with more than `merge_inline` (8) task partials are merged by k_msm_merge_heavy, one
// workgroup each; the others by the level-1 thread of the reduction (many jobs) or by one thread
// per bucket in the trailing workgroups of the same launch (few jobs, where level 1 is a latency chain)

// upper bound on the non-zero digits of one scalar: digits are >= c positions apart, 0 .. 254
__host__ ZK_DI uint32_t msm_max_digits(uint32_t c) { return 254 / c + 2; }

// the two-level counting sort (msm_sort.h)
constexpr uint32_t MSM_COARSE_MAX = 1024;      // coarse bins per job
constexpr uint32_t MSM_FINE_MAX = 2048;        // buckets per coarse bin
constexpr uint32_t MSM_COARSE_SCALARS = 1024;  // scalars per workgroup of passes 1 and 3 (4 per thread)
// threads of the one-workgroup kernels of the sort and of the task order
#ifdef ZK_EMU
constexpr uint32_t MSM_SORT_THREADS = 64;     // the test-only emulation runs one OS thread per GPU thread
#else
constexpr uint32_t MSM_SORT_THREADS = 1024;
#endif
constexpr uint32_t MSM_MERGE_THREADS = 256;   // k_msm_merge_heavy (msm_reduce.h)
constexpr uint32_t MSM_TABLE_CHUNK = 16;      // slices per inversion of k_msm_build_table (msm_point_kernels.h)

// Table multiples.  A table may hold, behind its 255 slices 2^k P, the slices of m 2^k P for the odd m = 3, 5, ... ,
// 2 n_mult - 1 (slice 255 j + k = m_j 2^k P, m_j = 2 j + 1).  The digit set grows to D = { +- m b : m = m_j, b odd,
// b < 2^(c-1) } over the SAME buckets - a digit m b goes into bucket b through the slice of m - so the zero runs between the
// digits grow.  At an odd residual k with more than W + 1 bits left (W = c + ext) the step is WIDE: for w = W down to c,
// rho = k mod 2^w and the candidates rho, rho - 2^w, the smaller magnitude first; the first candidate in D is the digit, its
// multiple the smallest m that divides it with a quotient below 2^(c-1), and the recoding goes on with (k - d) / 2^w (the
// carry stays 0 or 1).  w = c always finds the plain NAF digit.  Near the top of the scalar the step is the plain one of
// msm_wnaf.  The choice depends on the low W bits of the odd residual alone: lut[(k mod 2^W) >> 1] = (w - c) | negative
// candidate << 3 | j << 4, 2^(W-1) bytes per (c, n_mult, ext) that stay in L2 (msm_mult_choice makes them on the host).
constexpr uint32_t MSM_MULT_MAX = 8;
struct MsmRecode {
    const uint8_t* lut;     // null: one multiple, the plain msm_wnaf
    uint32_t n_mult, ext;
};
__host__ ZK_DI uint32_t msm_mult_ext(uint32_t n_mult) { return n_mult <= 1 ? 0u : n_mult == 2 ? 2u : 3u; }
// v: the low W = c + ext bits of an odd residual
__host__ ZK_DI uint8_t msm_mult_choice(uint32_t v, uint32_t c, uint32_t n_mult, uint32_t ext) {
    const uint32_t half = 1u << (c - 1);
    for (uint32_t w = c + ext; w >= c; w--) {
        const uint32_t rho = v & ((1u << w) - 1u), other = (1u << w) - rho;
        for (uint32_t t = 0; t < 2; t++) {
            const uint32_t negative = (rho < other) == (t == 0) ? 0u : 1u, mag = negative ? other : rho;
            for (uint32_t j = 0; j < n_mult; j++) {
                const uint32_t m = 2 * j + 1;
                if (mag % m == 0 && mag / m < half) return (uint8_t)((w - c) | (negative << 3) | (j << 4));
            }
        }
    }
    return 0;   // (not reached: at w = c the candidate of the smaller magnitude is below 2^(c-1))
}

// words of a field element in the host's layout (msm_points.h fld_import / fld_export), and whether its inversion has the
// Euclidean form (msm_inverse.h inv_gcd)
template <class F> struct HostWords;
template <> struct HostWords<Fq28> { static constexpr int N = 12; static constexpr bool GCD_INV = true; };
template <> struct HostWords<Fq2> { static constexpr int N = 24; static constexpr bool GCD_INV = false; };
template <> struct HostWords<Fq2x> { static constexpr int N = 24; static constexpr bool GCD_INV = true; };

}  // namespace zkdev
