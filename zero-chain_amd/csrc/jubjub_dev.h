// Jubjub on the device, one lane per point: the pieces of xt_inputs.h's IntoXY chain that other kernels share (redjubjub.h, ledger.h).
// Only ZK_DI functions and compile-time tables live here - no kernel, so a translation unit that includes this header
// compiles none: k_into_xy stays in xt_inputs.h, which verify.cpp alone includes.
//   Lds                      a lane's column of a block's LDS table, [slot][word][lane]
//   pow_windows              a^e for a constant exponent in fixed 4-bit windows (~330 dependent products for r - 2)
//   sqrt_one_pow             square root in Fr with ONE exponentiation, then Tonelli-Shanks (~290 + <= 500)
//   ext_dbl, cache_put, ext_add_cached   extended twisted Edwards, a = -1: dbl-2008-hwcd, addends cached as (Y + X, Y - X, 2 d T, 2 Z)
//   ext_add                  two extended points, add-2008-hwcd-3 (9 products): the operator of ledger.h's scan
//   ep_neutral, jubjub_d2, point_words, point_write   the neutral element, 2 d in Montgomery form, edwards::Point::write of an affine point
//   naf_chain                sum of signed odd digits times the cached P, 3P, 5P, 7P: 252 doublings, an addition per non-zero digit
//   is_prime_order           [s]P == O over the width-4 NAF of s recoded at compile time (~2 200)
//   mul_naf                  [k]P over a width-4 NAF recoded by the host at run time (elgamal_scan.h: ~2 400)
//   read_point               edwards::Point::read: y, and x by 1 / (d y^2 + 1) and the square root (~620)
#pragma once
#include "dev_field.h"
#include "consts.h"

namespace zkxt {

using zkdev::Fr;

enum { INTO_XY_OK = 0, INTO_XY_NOT_IN_FIELD = 1, INTO_XY_NOT_ON_CURVE = 2, INTO_XY_NOT_PRIME_ORDER = 3 };

// ---- the constant exponents and the group order, recoded at compile time
struct PowDigits {   // 4-bit windows, most significant first
    uint8_t d[64];
    int n;
};
constexpr PowDigits pow_digits(const uint32_t (&e)[8]) {
    PowDigits r{};
    bool started = false;
    for (int i = 63; i >= 0; i--) {
        const uint32_t v = (e[i >> 3] >> (4 * (i & 7))) & 15u;
        if (!started && !v) continue;
        started = true;
        r.d[r.n++] = (uint8_t)v;
    }
    return r;
}
constexpr PowDigits digits_inverse() {   // r - 2
    const uint32_t e[8] = ZK_FR_EXP_RM2_32;
    return pow_digits(e);
}
constexpr PowDigits digits_sqrt() {   // (q - 1) / 2 for r - 1 = 2^32 q: words 1 .. 7 of r, shifted down by one bit
    const uint32_t p[8] = ZK_FR_P_32;
    uint32_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 7; i++) e[i] = (p[i + 1] >> 1) | (i < 6 ? p[i + 2] << 31 : 0u);
    return pow_digits(e);
}
struct NafDigits {   // width-4 non-adjacent form of s, least significant first: odd digits in -7 .. 7
    int8_t d[256];
    int top;
};
constexpr NafDigits digits_order() {
    const uint64_t s[4] = ZK_JUBJUB_FS_MODULUS_64;
    uint64_t k[4] = {s[0], s[1], s[2], s[3]};
    NafDigits r{};
    for (int i = 0; i < 256; i++) {
        if (k[0] & 1u) {
            int v = (int)(k[0] & 15u);
            if (v >= 8) v -= 16;
            r.d[i] = (int8_t)v;
            r.top = i;
            if (v > 0) {
                k[0] -= (uint64_t)v;   // k is odd and v <= k[0] & 15: no borrow
            } else {
                const uint64_t a = (uint64_t)(-v), old = k[0];
                k[0] += a;
                if (k[0] < old)
                    for (int j = 1; j < 4 && ++k[j] == 0; j++) {}
            }
        }
        for (int j = 0; j < 4; j++) k[j] = (k[j] >> 1) | (j < 3 ? k[j + 1] << 63 : 0);
    }
    return r;
}

// ---- a lane's column of the block's LDS table: slot s, word w of this lane at (s * 8 + w) * 64
struct Lds {
    uint32_t* base;
    ZK_DI Fr ld(uint32_t slot) const {
        Fr r;
#pragma unroll
        for (int w = 0; w < 8; w++) r.l[w] = base[(slot * 8 + w) * 64];
        return r;
    }
    ZK_DI void st(uint32_t slot, const Fr& v) const {
#pragma unroll
        for (int w = 0; w < 8; w++) base[(slot * 8 + w) * 64] = v.l[w];
    }
};

// a^e for a constant exponent in 4-bit windows: slots 1 .. 15 hold a^1 .. a^15
ZK_DI Fr pow_windows(const Lds& L, const Fr& a, const PowDigits& e) {
    L.st(1, a);
    Fr p = a;
#pragma unroll 1
    for (uint32_t j = 2; j < 16; j++) {
        p = mul(p, a);
        L.st(j, p);
    }
    Fr r = L.ld(e.d[0]);
#pragma unroll 1
    for (int i = 1; i < e.n; i++) {
        r = sqr(sqr(sqr(sqr(r))));
        const uint32_t d = e.d[i];
        if (d) r = mul(r, L.ld(d));
    }
    return r;
}

// square root in Fr (2-adicity 32; any primitive 2^32-th root of unity serves, the caller fixes the sign): false if none
ZK_DI bool sqrt_one_pow(const Lds& L, const Fr& a, Fr* out) {
    if (a.is_zero()) {
        *out = a;
        return true;
    }
    constexpr PowDigits E = digits_sqrt();
    const Fr w = pow_windows(L, a, E);
    Fr x = mul(a, w), b = mul(x, w);   // a^((q + 1) / 2), a^q
    Fr z;
    {
        const uint32_t root[8] = ZK_FR_ROOT_OF_UNITY_MONT_32;
#pragma unroll
        for (int i = 0; i < 8; i++) z.l[i] = root[i];
    }
    const Fr one = Fr::one();
    uint32_t m = ZK_FR_S;
    while (b != one) {
        uint32_t k = 0;
        Fr t = b;
        while (t != one && k < m) {   // the order of b divides 2^32
            t = sqr(t);
            k++;
        }
        if (k >= m) break;   // a is no square: x^2 == a fails below
        Fr g = z;
        for (uint32_t j = 0; j + k + 1 < m; j++) g = sqr(g);
        x = mul(x, g);
        z = sqr(g);
        b = mul(b, z);
        m = k;
    }
    *out = x;
    return sqr(x) == a;
}

struct EP {   // extended twisted Edwards, a = -1
    Fr X, Y, Z, T;
};
ZK_DI EP ep_neutral() { return EP{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()}; }
// the curve's d and 2 d (the k of ext_add, cache_put), in Montgomery form
ZK_DI Fr jubjub_d() {
    Fr d;
    const uint64_t dp[4] = ZK_JUBJUB_D_PLAIN_64;
#pragma unroll
    for (int i = 0; i < 8; i++) d.l[i] = (uint32_t)(dp[i >> 1] >> (32 * (i & 1)));
    return zkdev::to_mont(d);
}
ZK_DI Fr jubjub_d2() { return dbl(jubjub_d()); }
// edwards::Point::write of an affine point in Montgomery form: y, the parity of x in the top bit - as 8 words, and into those at o
ZK_DI Fr point_words(const Fr& x_mont, const Fr& y_mont) {
    const Fr x = zkdev::from_mont(x_mont);
    Fr y = zkdev::from_mont(y_mont);
    y.l[7] |= (x.l[0] & 1u) << 31;
    return y;
}
ZK_DI void point_write(uint32_t* o, const Fr& x_mont, const Fr& y_mont) {
    const Fr y = point_words(x_mont, y_mont);
    uint4* q = reinterpret_cast<uint4*>(o);
    q[0] = make_uint4(y.l[0], y.l[1], y.l[2], y.l[3]);
    q[1] = make_uint4(y.l[4], y.l[5], y.l[6], y.l[7]);
}
// dbl-2008-hwcd, a = -1; T only where the next step reads it (an addition)
ZK_DI EP ext_dbl(const EP& p, bool want_t) {
    const Fr a = sqr(p.X), b = sqr(p.Y), c = dbl(sqr(p.Z));
    const Fr d = neg(a);
    const Fr e = sub(sub(sqr(add(p.X, p.Y)), a), b), g = add(d, b), f = sub(g, c), h = sub(d, b);
    EP r;
    r.X = mul(e, f);
    r.Y = mul(g, h);
    r.Z = mul(f, g);
    r.T = want_t ? mul(e, h) : Fr::zero();
    return r;
}
// a multiple of P as an addend: (Y + X, Y - X, 2 d T, 2 Z) in slots 4 i .. 4 i + 3
ZK_DI void cache_put(const Lds& L, uint32_t i, const EP& p, const Fr& d2) {
    L.st(4 * i, add(p.Y, p.X));
    L.st(4 * i + 1, sub(p.Y, p.X));
    L.st(4 * i + 2, mul(p.T, d2));
    L.st(4 * i + 3, dbl(p.Z));
}
// p + sign * cached[i] (add-2008-hwcd-3, unified and complete on this curve); T only where want_t
ZK_DI EP ext_add_cached(const Lds& L, const EP& p, uint32_t i, bool negative, bool want_t) {
    const Fr ypx = L.ld(4 * i + (negative ? 1 : 0)), ymx = L.ld(4 * i + (negative ? 0 : 1));
    const Fr a = mul(sub(p.Y, p.X), ymx), b = mul(add(p.Y, p.X), ypx);
    const Fr c = mul(p.T, L.ld(4 * i + 2)), d = mul(p.Z, L.ld(4 * i + 3));
    const Fr e = sub(b, a), h = add(b, a);
    const Fr f = negative ? add(d, c) : sub(d, c), g = negative ? sub(d, c) : add(d, c);
    EP r;
    r.X = mul(e, f);
    r.Y = mul(g, h);
    r.Z = mul(f, g);
    r.T = want_t ? mul(e, h) : Fr::zero();
    return r;
}
// p + q for two extended points (add-2008-hwcd-3 with k = 2 d: 9M; unified, and complete where both are of prime order)
ZK_DI EP ext_add(const EP& p, const EP& q, const Fr& d2) {
    const Fr a = mul(sub(p.Y, p.X), sub(q.Y, q.X)), b = mul(add(p.Y, p.X), add(q.Y, q.X));
    const Fr c = mul(mul(p.T, d2), q.T), d = dbl(mul(p.Z, q.Z));
    const Fr e = sub(b, a), f = sub(d, c), g = add(d, c), h = add(b, a);
    return EP{mul(e, f), mul(g, h), mul(f, g), mul(e, h)};
}
// P, 3P, 5P, 7P as addends in slots 0 .. 15
ZK_DI void cache_odd_multiples(const Lds& L, const EP& p1, const Fr& d2) {
    cache_put(L, 0, p1, d2);
    cache_put(L, 3, ext_dbl(p1, true), d2);   // 2P, in the place of 7P until 7P is written
    EP q = p1;
#pragma unroll 1
    for (uint32_t i = 1; i < 4; i++) {   // 3P, 5P, 7P = P, 3P, 5P + 2P
        q = ext_add_cached(L, q, 3, false, true);
        cache_put(L, i, q, d2);
    }
}
// sum_i digit(i) 2^i P over the cached multiples of P: digit(i) is 0 or odd in -7 .. 7 (a width-4 NAF), i = top .. 0, the same
// in every lane of the wave.  T of the result only where want_t.
template <class Digit>
ZK_DI EP naf_chain(const Lds& L, int top, Digit digit, bool want_t) {
    EP acc = ep_neutral();
#pragma unroll 1
    for (int i = top; i >= 0; i--) {
        const int v = digit(i);
        acc = ext_dbl(acc, v != 0 || (want_t && i == 0));
        if (v) acc = ext_add_cached(L, acc, (uint32_t)((v < 0 ? -v : v) >> 1), v < 0, want_t && i == 0);
    }
    return acc;
}
// [s](x, y) == O ?
ZK_DI bool is_prime_order(const Lds& L, const Fr& x, const Fr& y, const Fr& d2) {
    constexpr NafDigits S = digits_order();
    cache_odd_multiples(L, EP{x, y, Fr::one(), mul(x, y)}, d2);
    const EP acc = naf_chain(L, S.top, [&](int i) { return (int)S.d[i]; }, false);
    return acc.X.is_zero() && acc.Y == acc.Z;
}
// [k](x, y) in extended coordinates for a scalar the host recoded (d: its width-4 NAF, least significant first; top: the index
// of its last non-zero digit, -1 for k = 0).  Every lane of the wave reads the same digits: one chain shape for all.
ZK_DI EP mul_naf(const Lds& L, const Fr& x, const Fr& y, const Fr& d2, const int8_t* d, int top) {
    cache_odd_multiples(L, EP{x, y, Fr::one(), mul(x, y)}, d2);
    return naf_chain(L, top, [&](int i) { return (int)d[i]; }, true);
}

// edwards::Point::read (edwards.rs:92-165) of the encoding in the 8 words at enc: INTO_XY_OK, _NOT_IN_FIELD or _NOT_ON_CURVE.
// *y: the 255 bits as they came.  With OK also *x, plain like *y, both in Montgomery form (*xm, *ym) and the curve's d (*d).
ZK_DI uint32_t read_point(const Lds& L, const uint32_t* enc, Fr* x, Fr* y_out, Fr* xm_out, Fr* ym_out, Fr* d_out) {
    Fr y;
    {
        const uint4* q = reinterpret_cast<const uint4*>(enc);
        const uint4 lo = q[0], hi = q[1];
        y.l[0] = lo.x; y.l[1] = lo.y; y.l[2] = lo.z; y.l[3] = lo.w;
        y.l[4] = hi.x; y.l[5] = hi.y; y.l[6] = hi.z; y.l[7] = hi.w;
    }
    const bool sign = (y.l[7] >> 31) != 0;
    y.l[7] &= 0x7fffffffu;
    *y_out = y;
    {
        uint32_t bo = 0, co;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            (void)__builtin_subc(y.l[i], zkdev::FrCfg::P[i], bo, &co);
            bo = co;
        }
        if (bo == 0) return INTO_XY_NOT_IN_FIELD;
    }
    const Fr d = jubjub_d();
    const Fr ym = zkdev::to_mont(y);
    const Fr y2 = sqr(ym);
    constexpr PowDigits EI = digits_inverse();
    const Fr den_inv = pow_windows(L, add(mul(d, y2), Fr::one()), EI);   // d y^2 + 1 = 0 has no solution
    const Fr x2 = mul(sub(y2, Fr::one()), den_inv);
    Fr xm;
    if (!sqrt_one_pow(L, x2, &xm)) return INTO_XY_NOT_ON_CURVE;
    *x = zkdev::from_mont(xm);
    if (((x->l[0] & 1u) != 0) != sign) {
        xm = neg(xm);
        *x = neg(*x);
    }
    *xm_out = xm;
    *ym_out = ym;
    *d_out = d;
    return INTO_XY_OK;
}

}  // namespace zkxt
