// Points in and out, kernels (overview: msm.h): import, decoding and validation of bases, the table of doublings and
// multiples, export and normalisation of results.  All templates over the field: a unit compiles what it launches.
#pragma once
#include "msm_inverse.h"
#include "msm_points.h"

namespace zkdev {

template <class F>
static __global__ void __launch_bounds__(128)
k_import_affine(const uint32_t* __restrict__ src, Affine<F>* dst, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int W = HostWords<F>::N;
    Affine<F> p;
    fld_import(p.x, src + (size_t)i * 2 * W);
    fld_import(p.y, src + (size_t)i * 2 * W + W);
    dst[i] = p;
}
// ---------------------------------------------------------------------------------------------
// Point decoding on the device: the uncompressed encodings of the reference (G1: x | y, ec.rs:666-753; G2: x.c1 | x.c0 |
// y.c1 | y.c0, ec.rs:1303-1427; 48-byte big-endian coordinates, three flag bits on top of the first) -> affine table
// entries in the kernels' field representation.  What `into_affine_unchecked` accepts is accepted: the compression flag and
// the sort flag must be clear, the infinity flag demands an otherwise all-zero encoding (-> (0, 0), map = -1: a legal
// multiexp base that contributes nothing), every coordinate must be < q.  Membership of the curve and of the subgroup is
// k_check_points' business.  The host decoders (host_math.h g1_from_uncompressed / g2_from_uncompressed) give the same
// verdicts; they cost 0.11 s for 2^20 points on one core where this kernel takes 0.1 ms.
// stat[0] = smallest index of a refused encoding (0xffffffff: none), stat[1] = points at infinity met.
// ---------------------------------------------------------------------------------------------
template <class F>
static __global__ void __launch_bounds__(128)
k_decode_uncompressed(const uint32_t* __restrict__ src, Affine<F>* dst, int32_t* map, uint32_t* stat, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int W = HostWords<F>::N;                  // 12 / 24 words per coordinate
    const uint32_t* p = src + (size_t)i * 2 * W;
    const uint32_t flags = zk_bswap32(p[0]) >> 29;      // bit 2: compressed, bit 1: infinity, bit 0: sort (ec.rs:666-700)
    Affine<F> a;
    uint32_t any = 0;
    const bool okx = fld_decode(a.x, p, true, any);
    const bool oky = fld_decode(a.y, p, false, any);
    bool bad = (flags & 4u) != 0;
    bool inf = false;
    if (!bad) {
        if (flags & 2u) {
            bad = (flags & 1u) != 0 || any != 0;        // the infinity encoding is 0x40 followed by zeros
            inf = !bad;
        } else {
            bad = (flags & 1u) != 0 || !okx || !oky;
        }
    }
    if (bad || inf) a = Affine<F>{F::zero(), F::zero()};
    dst[i] = a;
    if (map) map[i] = inf || bad ? -1 : (int32_t)i;
    if (bad) atomicMin(&stat[0], i);
    if (inf) atomicAdd(&stat[1], 1u);
}

template <class F>
static __global__ void __launch_bounds__(64)
k_export_xyzz(const XYZZ<F>* __restrict__ src, uint32_t* dst, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int W = HostWords<F>::N;
    XYZZ<F> p = src[i];
    fld_export(p.x, dst + (size_t)i * 4 * W);
    fld_export(p.y, dst + (size_t)i * 4 * W + W);
    fld_export(p.zz, dst + (size_t)i * 4 * W + 2 * W);
    fld_export(p.zzz, dst + (size_t)i * 4 * W + 3 * W);
}

// ---------------------------------------------------------------------------------------------
// Final fold of a proof on the GPU (bellman prover.rs: g_c = s * g_a + ..., then into_affine of A, B,
// C).  On the host it cost 0.47 ms per proof - a 255-bit double-and-add plus three field inversions
// - i.e. 30 ms per 1024-proof chunk on 16 cores with the GPU idle (8 % of the step).  The fold itself
// is coop_tail.cpp's k_ct_scale_add; the conversions to affine form are here.
// ---------------------------------------------------------------------------------------------
// dst[i] = src[i] in affine form, exported in the host's XYZZ layout with zz = zzz = 1 (all zero for
// the point at infinity): the host only has to encode it.
template <class F, bool GCD>
ZK_DI void xyzz_normalize_export(const XYZZ<F>* __restrict__ src, uint32_t* dst, uint32_t i) {
    constexpr int W = HostWords<F>::N;
    const XYZZ<F> p = src[i];
    const bool inf = p.is_inf();
    const Affine<F> a = to_affine<F, GCD && HostWords<F>::GCD_INV>(p);
    const F unit = inf ? F::zero() : F::one();
    fld_export(a.x, dst + (size_t)i * 4 * W);
    fld_export(a.y, dst + (size_t)i * 4 * W + W);
    fld_export(unit, dst + (size_t)i * 4 * W + 2 * W);
    fld_export(unit, dst + (size_t)i * 4 * W + 3 * W);
}
template <class F, bool GCD>
static __global__ void __launch_bounds__(64, MsmOcc<F>::tail)
k_xyzz_normalize_export(const XYZZ<F>* __restrict__ src, uint32_t* dst, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xyzz_normalize_export<F, GCD>(src, dst, i);
}
// the same for two arrays in one launch (A and C of a proof made alone: side by side instead of one after the other)
template <class F, bool GCD>
static __global__ void __launch_bounds__(64, MsmOcc<F>::tail)
k_xyzz_normalize_export2(const XYZZ<F>* __restrict__ src0, const XYZZ<F>* __restrict__ src1, uint32_t* dst0, uint32_t* dst1, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    if (i < n) xyzz_normalize_export<F, GCD>(src0, dst0, i);
    else xyzz_normalize_export<F, GCD>(src1, dst1, i - n);
}

// flags[i] bit0: not on curve, bit1: not in the r-torsion subgroup.  Infinity ((0,0)) passes.
// The subgroup test is the reference's (ec.rs:142-144): r * P == infinity.
template <class F>
static __global__ void __launch_bounds__(128)
k_check_points(const Affine<F>* __restrict__ pts, uint32_t n, uint32_t do_subgroup, uint32_t* flags) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = pts[i];
    uint32_t f = 0;
    if (!p.is_inf()) {
        F lhs = sqr(p.y);
        F rhs = add(mul(sqr(p.x), p.x), curve_b((const F*)nullptr));   // < 2 MO
        if (!is_zero_full(sub_b<2 * F::MO>(lhs, rhs))) f |= 1u;
        if (do_subgroup && !f) {
            const uint32_t r[8] = ZK_FR_P_32;
            XYZZ<F> acc = XYZZ<F>::inf();
            for (int w = 7; w >= 0; w--)
                for (int b = 31; b >= 0; b--) {
                    acc = xdbl(acc);
                    if ((r[w] >> b) & 1u) madd(acc, p, false);
                }
            if (!acc.is_inf()) f |= 2u;
        }
    }
    flags[i] = f;
}

// ---------------------------------------------------------------------------------------------
// Table construction: table[k][i] = 2^k * P_i  (affine), k < MSM_NPOS, plus validity checks.
// ---------------------------------------------------------------------------------------------
// One thread per base point walks the doubling chain in extended-Jacobian form and brings the slices
// to affine form MSM_TABLE_CHUNK at a time with ONE field inversion per chunk (Montgomery's trick:
// prefix products of the zzz, one inversion, back-substitution) - ~54 field products per table entry
// instead of one Fermat inversion (~590) each.  `scratch` holds 5 field elements per chunk slot and
// point, [slot][field][point].  Points at infinity (legal bases, mapped out) and - for unchecked keys
// - a chain that runs into infinity are carried through as (0, 0).
// n_mult > 1: behind the 255 slices of P those of 3 P, 5 P, ... (slice 255 j + k = (2 j + 1) 2^k P): 3 P = 2 P + P,
// 5 P = 3 P + 2 P, ... with the complete addition, then the same chain per multiple over the same scratch.  j0: the first
// multiple whose slices are made (the ones before it are in place: MsmGroup::add_multiples).
template <class F>
static __global__ void __launch_bounds__(128)
k_msm_build_table(Affine<F>* table, uint32_t n, uint32_t npos, F* scratch, uint32_t n_mult, uint32_t j0) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p0 = table[i];   // slice 0 was uploaded by the host
    XYZZ<F> mult = p0.is_inf() ? XYZZ<F>::inf() : XYZZ<F>{p0.x, p0.y, F::one(), F::one()};
    const XYZZ<F> two = n_mult > 1 ? xdbl(mult) : XYZZ<F>::inf();
    auto slot = [&](uint32_t j, uint32_t f) -> F& { return scratch[((size_t)j * 5 + f) * n + i]; };
    for (uint32_t jm = 0; jm < n_mult; jm++) {
        if (jm) mult = xadd(mult, two);
        if (jm < j0) continue;
        XYZZ<F> cur = mult;
        Affine<F>* tj = table + (size_t)jm * npos * n;
        for (uint32_t k0 = jm ? 0u : 1u; k0 < npos; k0 += MSM_TABLE_CHUNK) {   // (slice 0 of a multiple is the multiple itself)
            const uint32_t nc = npos - k0 < MSM_TABLE_CHUNK ? npos - k0 : MSM_TABLE_CHUNK;
            F run = F::one();
            for (uint32_t j = 0; j < nc; j++) {
                if (k0 + j) cur = xdbl(cur);
                slot(j, 0) = cur.x;
                slot(j, 1) = cur.y;
                slot(j, 2) = cur.zz;
                slot(j, 3) = cur.zzz;
                slot(j, 4) = run;                                   // product of the zzz before this one
                if (!cur.is_inf()) run = mul(run, cur.zzz);
            }
            F inv_run = inv_fast(run);
            for (uint32_t j = nc; j-- > 0;) {
                const XYZZ<F> q{slot(j, 0), slot(j, 1), slot(j, 2), slot(j, 3)};
                Affine<F> a{F::zero(), F::zero()};
                if (!q.is_inf()) {
                    const F izzz = mul(inv_run, slot(j, 4));
                    inv_run = mul(inv_run, q.zzz);
                    const F izz = mul(sqr(q.zz), sqr(izzz));       // zz^2 / zzz^2 = 1 / zz
                    a = Affine<F>{mul(q.x, izz), mul(q.y, izzz)};
                }
                tj[(size_t)(k0 + j) * n + i] = a;
            }
        }
    }
}

}  // namespace zkdev
