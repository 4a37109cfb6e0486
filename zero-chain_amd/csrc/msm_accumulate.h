// Pass 5 of the multiexp (overview: msm.h): the compiled accumulation of a task's points, its second pass over the tasks the
// generated loops flag, what the wrappers of those loops share (msm_asm_g1.h, msm_asm_g2.h), and the synthetic inputs of
// the load-time comparison of their forms.
#pragma once
#include "dev_curve.h"
#include "msm_types.h"

namespace zkdev {

// Pass 5: one thread per task (= at most seg points of one bucket), tasks in length order.
// Two things measured NOT to matter here, neither in the batched prover (4 GB of tables) nor on one
// 2^20-point job (30 GB): fetching the next point while the current one is added (28 more live
// registers; measured again in round 2 as a two-deep pipeline with the pair index two steps ahead: G1
// 176.6 -> 178.4 ms per launch, G2 at one wave per SIMD 93.2 -> 91.2: kept there only), and sorting every task's pairs by table index so that all
// lanes sweep the doubling slices in step.  What bounds the issue rate at two waves per SIMD is the product
// routine itself (66 G products/s at this occupancy against 74.5 at eight waves, profiles/r01f_ubench.txt);
// three waves per SIMD (168 VGPRs, 88 bytes of scratch per lane) measured 179.6 ms, four (128 VGPRs) 237.7.
// The single job's lower rate (4.3 G additions/s against 7.0) is 88 % occupancy at
// the two ends of a 3 ms launch, a 12 % lower issue rate per resident wave and a lower clock.
template <class F, int OCC, bool PIPELINED = false>
ZK_DI void msm_accumulate_body(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ pairs,
                               const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<F>* __restrict__ tsums) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total[0]) return;
    const uint4 d = sorted[t];
    const uint32_t o = d.x, n = d.z;
    XYZZ<F> acc = XYZZ<F>::inf();
    if (PIPELINED && n) {
        // one wave per SIMD has nobody to hide a gather behind: the pair index two steps ahead and the table entry
        // one step ahead are in flight while the current entry is added (steps past the end re-read the last pair)
        const uint32_t last = n - 1;
        uint32_t pr = pairs[o];
        uint32_t pr_n = pairs[o + (1u < last ? 1u : last)];
        Affine<F> p = table[pr >> 1];
        for (uint32_t k = 0; k < n; k++) {
            const Affine<F> p_n = table[pr_n >> 1];
            const uint32_t pr_nn = pairs[o + (k + 2 < last ? k + 2 : last)];
            madd(acc, p, (pr & 1u) != 0);
            p = p_n;
            pr = pr_n;
            pr_n = pr_nn;
        }
    } else {
        for (uint32_t k = 0; k < n; k++) {
            uint32_t pr = pairs[o + k];
            Affine<F> p = table[pr >> 1];
            madd(acc, p, (pr & 1u) != 0);
        }
    }
    tsums[d.y] = acc;
}
template <class F>
static __global__ void __launch_bounds__(128, MsmOcc<F>::acc)
k_msm_accumulate(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ pairs,
                 const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<F>* __restrict__ tsums) {
    msm_accumulate_body<F, MsmOcc<F>::acc>(table, pairs, sorted, total, tsums);
}
// the same at one wave per SIMD: the whole register file (256 VGPRs + 256 AGPRs) for one wave, i.e. an Fq2
// accumulator (112 registers) plus the fused product's working set without scratch traffic
template <class F>
static __global__ void __launch_bounds__(128, 1)
k_msm_accumulate_wide(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ pairs,
                      const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<F>* __restrict__ tsums) {
    msm_accumulate_body<F, 1, true>(table, pairs, sorted, total, tsums);
}

// Second pass for the tasks the assembly loop flagged: the compiled addition with every special case.  A circuit's
// CRS holds EQUAL points (variables with identical QAP polynomials); the jobs of a proof take each group of them as ONE
// term under the sum of its scalars (zkamd.cpp ensure_maps), so two equal table entries meet in a task only by coincidence,
// under ZKAMD_MERGE_BASES=0 (~100-170 flagged tasks per 1024-proof launch of the transfer circuit, each time a task
// starts with two of them) or in a caller's own bases.  One WAVE per flagged task - lane l sums the points k = l (mod 64)
// of the task, an LDS tree adds the 64 partial sums - instead of one thread walking up to 256 points behind everybody
// else (9.4 + 3.2 ms per chunk before, r03final trace).
template <class F>
static __global__ void __launch_bounds__(64, 1)
k_msm_accumulate_redo(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ pairs, const uint4* __restrict__ sorted,
                      const uint32_t* __restrict__ n_redo, const uint32_t* __restrict__ redo, XYZZ<F>* __restrict__ tsums) {
    ZK_SHARED XYZZ<F> sm[64];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n_redo[0]; i += gridDim.x) {
        const uint4 d = sorted[redo[i]];
        XYZZ<F> acc = XYZZ<F>::inf();
        for (uint32_t k = lane; k < d.z; k += 64) {
            const uint32_t pr = pairs[d.x + k];
            const Affine<F> p = table[pr >> 1];
            madd(acc, p, (pr & 1u) != 0);
        }
        sm[lane] = acc;
        __syncthreads();
        for (uint32_t st = 32; st >= 1; st >>= 1) {
            if (lane < st) sm[lane] = xadd(sm[lane], sm[lane + st]);
            __syncthreads();
        }
        if (lane == 0) tsums[d.y] = sm[0];
        __syncthreads();
    }
}

#ifdef ZK_HAVE_MADD_ASM
// Shared by the wrappers of the generated loops: a coordinate of the signed loops back in the unsigned form of dev_field.h,
// and the lane index from the execution mask (the scratch-free second forms).
// a product of the signed loop: digits exactly normalised, top limb possibly negative, value in (-0.07 p, 2 p) -> [0, 2 p)
// (`z`: a zero the compiler cannot see through, taken AFTER an assembly loop - the scratch-free second forms of the kernels
//  below pass it so that no constant of the conversion is hoisted across a loop that owns every VGPR, i.e. into scratch)
ZK_DI Fq28 fq28_from_signed_product(const u32x16& v, uint32_t z = 0) {
    Fq28 r = fq28_unvec(v);
    if ((int32_t)r.l[13] < 0) {
        uint32_t c = z;
#pragma unroll
        for (int i = 0; i < 13; i++) {
            const uint32_t t = r.l[i] + Fq28Consts::P[i] + c;
            r.l[i] = t & FQ28_MASK;
            c = t >> 28;
        }
        r.l[13] += Fq28Consts::P[13] + c;
    }
    return r;
}
// spread(M) +- a signed lazy value (limbs above -(3 * 2^28 - 3)): the unsigned weakly normalised form, value < (M + 2) p
template <int M, bool NEGATE>
ZK_DI Fq28 fq28_from_signed(const u32x16& v, uint32_t z = 0) {
    Fq28 r;
#pragma unroll
    for (int i = 0; i < 14; i++) r.l[i] = NEGATE ? (Fq28Spread<M>::V[i] + z) - v[i] : (Fq28Spread<M>::V[i] + z) + v[i];
    fq28_wnorm(r.l);
    return r;
}
ZK_DI uint32_t lane_of_wave(uint32_t z) { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)); }
#endif

// Synthetic inputs for the load-time comparison of the two forms of the scratch-using kernels (zkamd.cpp
// calibrate_kernel_forms): `ntasks` accumulation tasks of `len` pairs each over pseudo-random entries of a real table, and
// bucket sums that are real points of a real table.
ZK_DI uint32_t calib_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
template <class F>
static __global__ void __launch_bounds__(256)
k_calib_buckets(const Affine<F>* __restrict__ table, uint32_t n_table, XYZZ<F>* sums, uint32_t n_sums, uint32_t* cnt, uint32_t* toff,
                uint32_t n_buckets) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sums) sums[i] = XYZZ<F>::from_affine(table[calib_hash(i) % n_table]);
    if (i < n_buckets) {
        cnt[i] = 1;
        toff[i] = calib_hash(i ^ 0x5bd1e995u) % n_sums;
    }
}

}  // namespace zkdev
