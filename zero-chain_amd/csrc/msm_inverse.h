// Field inversion on the device (overview: msm.h) and the affine form of a point.  Device functions only: the table builder
// and the normalisation (msm_point_kernels.h), the pairing kernels (pairing.h) and parameter generation (setup.h) call them.
#pragma once
#include "dev_curve.h"
#include "coop_inv.h"

namespace zkdev {

// a^(q - 2) by square-and-multiply, MSB first (off the hot path: table construction, affine conversion).  The
// loops stay ROLLED: unrolled over the constant exponent they are 380 call sites per use and most of the library's
// compile time.  (As an out-of-line function it measured 4x slower: table build 0.31 -> 1.29 s for 2^20 bases.)
#define ZK_POW_ATTR ZK_DI   // inlined, but with ROLLED loops (the unrolled form is what cost the compile time)
template <class F>
ZK_POW_ATTR F fq_pow_qm2(const F& a) {
    const uint32_t e[12] = ZK_FQ_EXP_QM2_32;
    F r = a;
    bool started = false;
#pragma unroll 1
    for (int i = 11; i >= 0; i--) {
        const uint32_t w = e[i];
#pragma unroll 1
        for (int b = 31; b >= 0; b--) {
            if (started) r = sqr(r);
            if ((w >> b) & 1u) {
                if (started) r = mul(r, a);
                started = true;
            }
        }
    }
    return r;
}
// the unrolled form (the exponent's bits become straight-line code): 2.4x faster than the rolled loop, paid for in
// compile time - used where inversions dominate a kernel (k_msm_build_table: one per 16 table entries)
template <class F>
ZK_DI F fq_pow_qm2_unrolled(const F& a) {
    const uint32_t e[12] = ZK_FQ_EXP_QM2_32;
    F r = a;
    bool started = false;
    for (int i = 11; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            if (started) r = sqr(r);
            if ((e[i] >> b) & 1u) {
                if (started) r = mul(r, a);
                started = true;
            }
        }
    return r;
}
// a^-1 by the binary extended Euclidean algorithm on the canonical integer (no products: ~760 shift / subtract steps
// of 12 words) - for kernels where ONE thread inverts ONE element and the chain of 570 dependent products of the
// Fermat form is the whole run time (the final into_affine of a proof made alone: 0.66 -> 0.1 ms).  Divergent
// loops: not for kernels with a full machine of lanes.  inv_gcd(0) = 0.
// y = u^-1 mod q for a canonical integer 0 < u < q (12 little-endian words); u is consumed
ZK_DI void gcd_inv_words_binary(uint32_t (&u)[12], uint32_t (&y)[12]) {
    uint32_t v[12], x1[12], x2[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        v[i] = FqCfg::P[i];
        x1[i] = i == 0 ? 1u : 0u;
        x2[i] = 0;
    }
    auto is_one = [](const uint32_t (&w)[12]) {
        uint32_t r = w[0] ^ 1u;
#pragma unroll
        for (int i = 1; i < 12; i++) r |= w[i];
        return r == 0;
    };
    auto shr1 = [](uint32_t (&w)[12]) {
#pragma unroll
        for (int i = 0; i < 11; i++) w[i] = (w[i] >> 1) | (w[i + 1] << 31);
        w[11] >>= 1;
    };
    auto halve_mod = [&](uint32_t (&w)[12]) {   // w / 2 mod p: w < p < 2^381, so w + p fits the 12 words
        if (w[0] & 1u) {
            uint32_t cy = 0, co;
#pragma unroll
            for (int i = 0; i < 12; i++) {
                w[i] = __builtin_addc(w[i], FqCfg::P[i], cy, &co);
                cy = co;
            }
        }
        shr1(w);
    };
    auto geq = [](const uint32_t (&a_)[12], const uint32_t (&b_)[12]) {
        uint32_t bo = 0, co;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            (void)__builtin_subc(a_[i], b_[i], bo, &co);
            bo = co;
        }
        return bo == 0;
    };
    auto sub = [](uint32_t (&a_)[12], const uint32_t (&b_)[12]) {   // a -= b, returns the borrow
        uint32_t bo = 0, co;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            a_[i] = __builtin_subc(a_[i], b_[i], bo, &co);
            bo = co;
        }
        return bo;
    };
    auto sub_mod = [&](uint32_t (&a_)[12], const uint32_t (&b_)[12]) {
        if (sub(a_, b_)) {
            uint32_t cy = 0, co;
#pragma unroll
            for (int i = 0; i < 12; i++) {
                a_[i] = __builtin_addc(a_[i], FqCfg::P[i], cy, &co);
                cy = co;
            }
        }
    };
    while (!is_one(u) && !is_one(v)) {
        while (!(u[0] & 1u)) {
            shr1(u);
            halve_mod(x1);
        }
        while (!(v[0] & 1u)) {
            shr1(v);
            halve_mod(x2);
        }
        if (geq(u, v)) {
            sub(u, v);
            sub_mod(x1, x2);
        } else {
            sub(v, u);
            sub_mod(x2, x1);
        }
    }
    const bool first = is_one(u);
#pragma unroll
    for (int i = 0; i < 12; i++) y[i] = first ? x1[i] : x2[i];
}
// ... and since round 6 by the half-GCD of coop_inv.h (batches of 30 division steps on the low limbs, transition matrices
// applied with 64-bit accumulators: ~25 batches of ~500 instructions instead of ~760 twelve-word shift / subtract steps);
// the binary form above stays as the emulation's cross-check.
ZK_DI void gcd_inv_words(uint32_t (&u)[12], uint32_t (&y)[12]) {
    gcd_inverse_words(u, y);
#ifdef ZK_EMU
    uint32_t y2[12];
    gcd_inv_words_binary(u, y2);
    for (int i = 0; i < 12; i++)
        if (y[i] != y2[i]) {
            fprintf(stderr, "gcd_inv_words: the half-GCD and the binary algorithm disagree\n");
            abort();
        }
#endif
}
ZK_DI Fq28 inv_gcd(const Fq28& a) {
    uint32_t u[12], y[12];
    fq28_export(a, u);   // x * 2^384 mod p, canonical
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) any |= u[i];
    if (!any) return Fq28::zero();
    gcd_inv_words(u, y);
    // (x * 2^384)^-1 as an integer -> x^-1 in the device's Montgomery form
    return mul(fq28_unpack(y), Fq28::from_const(Fq28Consts::KINV));
}
// the same for the saturated representation (the pairing kernels): a.l = x R canonical, (x R)^-1 R^3 / R = x^-1 R
ZK_DI Fq32 inv_gcd(const Fq32& a) {
    uint32_t u[12], y[12];
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        u[i] = a.l[i];
        any |= u[i];
    }
    if (!any) return Fq32::zero();
    gcd_inv_words(u, y);
    const uint32_t r3[12] = ZK_FQ_R3_32;
    Fq32 t, k;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        t.l[i] = y[i];
        k.l[i] = r3[i];
    }
    return mul(t, k);
}
ZK_DI Fq2x inv_gcd(const Fq2x& a) {
    Fq28 n = add(sqr(a.c0), sqr(a.c1));
    Fq28 t = inv_gcd(n);
    return Fq2x{mul(a.c0, t), neg_b<2>(mul(a.c1, t))};
}
ZK_DI Fq28 inv_fast(const Fq28& a) { return fq_pow_qm2_unrolled(a); }
ZK_DI Fq28 inv(const Fq28& a) { return fq_pow_qm2(a); }
ZK_DI Fq32 inv(const Fq32& a) { return fq_pow_qm2(a); }
ZK_DI Fq2x inv(const Fq2x& a) {
    // fq2.rs:160-176
    Fq28 n = add(sqr(a.c0), sqr(a.c1));
    Fq28 t = inv(n);
    return Fq2x{mul(a.c0, t), neg_b<2>(mul(a.c1, t))};
}
ZK_DI Fq32 inv_fast(const Fq32& a) { return fq_pow_qm2(a); }
ZK_DI Fq2x inv_fast(const Fq2x& a) {
    Fq28 n = add(sqr(a.c0), sqr(a.c1));
    Fq28 t = inv_fast(n);
    return Fq2x{mul(a.c0, t), neg_b<2>(mul(a.c1, t))};
}
ZK_DI Fq2 inv(const Fq2& a) {
    // fq2.rs:160-176
    Fq32 n = add(sqr(a.c0), sqr(a.c1));
    Fq32 t = inv(n);
    return Fq2{mul(a.c0, t), neg(mul(a.c1, t))};
}

ZK_DI Fq2 inv_fast(const Fq2& a) { return inv(a); }   // saturated G2 (A/B builds only)

template <class F, bool GCD = false>
ZK_DI Affine<F> to_affine(const XYZZ<F>& p) {
    if (p.is_inf()) return Affine<F>{F::zero(), F::zero()};
    F izzz;
    if constexpr (GCD) izzz = inv_gcd(p.zzz);
    else izzz = inv(p.zzz);
    F izz = mul(sqr(p.zz), sqr(izzz));   // zz^2 / zzz^2 = 1 / zz
    return Affine<F>{mul(p.x, izz), mul(p.y, izzz)};
}

}  // namespace zkdev
