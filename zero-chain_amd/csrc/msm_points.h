// Points in and out, device functions (overview: msm.h): the curve constant, the host's layout of a field element, the
// reference's big-endian encodings.  The kernels over them are msm_point_kernels.h.
#pragma once
#include "dev_curve.h"
#include "msm_types.h"

namespace zkdev {

ZK_DI Fq28 curve_b(const Fq28*) { return Fq28::from_const(Fq28Consts::B); }
ZK_DI Fq32 curve_b32() {
    Fq32 b;
    const uint32_t v[12] = ZK_FQ_B_MONT_32;
#pragma unroll
    for (int i = 0; i < 12; i++) b.l[i] = v[i];
    return b;
}
ZK_DI Fq2x curve_b(const Fq2x*) {
    Fq28 b = Fq28::from_const(Fq28Consts::B);
    return Fq2x{b, b};   // 4(u + 1), ec.rs:1567-1572
}
ZK_DI Fq2 curve_b(const Fq2*) {
    Fq32 b = curve_b32();
    return Fq2{b, b};   // 4(u + 1), ec.rs:1567-1572
}

// Host interchange.  The host side (host_math.h) and the C ABI speak the reference's layout:
// 6 x u64 Montgomery limbs per Fq (fq.rs:700-701), c0 then c1 for Fq2.  G1 is converted to /
// from the device's Fq28 by these kernels; for G2 they are plain copies.
ZK_DI void fld_import(Fq28& d, const uint32_t* h) { d = fq28_import(h); }
ZK_DI void fld_export(const Fq28& d, uint32_t* h) { fq28_export(d, h); }
ZK_DI void fld_import(Fq2& d, const uint32_t* h) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
        d.c0.l[i] = h[i];
        d.c1.l[i] = h[12 + i];
    }
}
ZK_DI void fld_export(const Fq2& d, uint32_t* h) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
        h[i] = d.c0.l[i];
        h[12 + i] = d.c1.l[i];
    }
}
ZK_DI void fld_import(Fq2x& d, const uint32_t* h) {
    d.c0 = fq28_import(h);
    d.c1 = fq28_import(h + 12);
}
ZK_DI void fld_export(const Fq2x& d, uint32_t* h) {
    fq28_export(d.c0, h);
    fq28_export(d.c1, h + 12);
}

ZK_DI uint32_t zk_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// 48 big-endian bytes at src (12 words as a little-endian load sees them) -> the integer's 12 little-endian words;
// all_zero &= (value == 0), the return value is (value < q)
ZK_DI bool be48_words(const uint32_t* __restrict__ src, uint32_t (&w)[12], uint32_t first_word_mask, uint32_t& any) {
    const uint4* q = reinterpret_cast<const uint4*>(src);
    const uint4 a = q[0], b = q[1], c = q[2];
    const uint32_t in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 12; i++) w[i] = zk_bswap32(in[11 - i]);
    w[11] &= first_word_mask;
    uint32_t o = 0, bo = 0, co;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        o |= w[i];
        (void)__builtin_subc(w[i], FqCfg::P[i], bo, &co);
        bo = co;
    }
    any |= o;
    return bo != 0;   // a borrow out of w - q: w < q
}
ZK_DI void fld_from_canon(Fq28& d, const uint32_t (&w)[12]) { d = mul(fq28_unpack(w), Fq28::from_const(Fq28Consts::R2)); }
ZK_DI void fld_from_canon(Fq32& d, const uint32_t (&w)[12]) {
    Fq32 v;
#pragma unroll
    for (int i = 0; i < 12; i++) v.l[i] = w[i];
    d = mul(v, Fq32::r2());
}
// one field element of the encoding at src (advanced past it); `first`: it carries the flag bits (masked off here)
ZK_DI bool fld_decode(Fq28& d, const uint32_t*& src, bool first, uint32_t& any) {
    uint32_t w[12];
    const bool ok = be48_words(src, w, first ? 0x1fffffffu : 0xffffffffu, any);
    src += 12;
    fld_from_canon(d, w);
    return ok;
}
template <class F2>
ZK_DI bool fld_decode_fq2(F2& d, const uint32_t*& src, bool first, uint32_t& any) {
    uint32_t w1[12], w0[12];
    const bool ok1 = be48_words(src, w1, first ? 0x1fffffffu : 0xffffffffu, any);   // c1 first (ec.rs:1408-1426)
    const bool ok0 = be48_words(src + 12, w0, 0xffffffffu, any);
    src += 24;
    fld_from_canon(d.c1, w1);
    fld_from_canon(d.c0, w0);
    return ok1 && ok0;
}
ZK_DI bool fld_decode(Fq2x& d, const uint32_t*& src, bool first, uint32_t& any) { return fld_decode_fq2(d, src, first, any); }
ZK_DI bool fld_decode(Fq2& d, const uint32_t*& src, bool first, uint32_t& any) { return fld_decode_fq2(d, src, first, any); }

}  // namespace zkdev
