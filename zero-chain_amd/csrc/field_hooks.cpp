// Test hook for the device field arithmetic and the XYZZ group law, one element per lane (tests/field_cases.py,
// tests/test_field_ops.py) and one element per DPP row (tests/coop_cases.py, tests/test_coop_field_ops.py).
// The whole unit is compiled only under -DZK_TEST_HOOKS (libzkamd_hooks.so, the emulation build): in the shipped library it
// is an empty object, and zk_hook_field_op is not part of include/zkamd.h.
#ifdef ZK_TEST_HOOKS
#include "host_common.h"
#include "dev_curve.h"
#include "coop_curve.h"

// One thread per row applies ONE function of dev_field.h / dev_curve.h to the limbs of its row as they are: no import, no
// reduction, no check of any bound, so the caller decides every limb of every operand (values at the edge of their bound,
// limbs at exactly 2^28 + 8, un-normalised operands, multiples of p).  The hook calls the same ZK_DI functions the product
// kernels call, so the out-of-line and naked assembly routines they reach (mul_asm.h FQ28, FQ28SQR, FQ28MAC2, FQ2MUL28,
// FQ28MUL2, and the saturated FR / FQ products) are byte-identical to the product's; only the calling context - what the
// compiler has in which register around the call - differs.  Blocks are 64 threads: the 64 lanes of a wave hold 64
// different rows, and a row count that is no multiple of 64 runs the routines under a partial EXEC mask.
//
// Layout.  A row of `in` is NI slots, a row of `out` NO slots, a slot is 16 words: the 14 limbs of an Fq28 and 2 pad words
// (ignored on input, zero on output).  An Fq2x is two slots (c0, c1); an affine point x, y; an XYZZ point x, y, zz, zzz.
// A value of the saturated fields (Fp<FrCfg>: 8 words, Fp<FqCfg>: 12 words) and the 12 host words of unpack / import /
// export sit in the low words of their slot.  A truth value is word 0 of its slot.
//
//   op family (in -> out slots)                                      the function
//   FQ28_ADD (2 -> 1), FQ28_DBL (1 -> 1)                             add, dbl
//   FQ28_SUB_B_<B> (2 -> 1), FQ28_NEG_B_<B> (1 -> 1)                 sub_b<B>, neg_b<B>      B = 2 4 5 7 10 15 63
//   FQ28_SUB_RAW_<B> (2 -> 1), FQ28_NEG_RAW_<B> (1 -> 1)             sub_raw<B>, neg_raw<B>  (MO, 2 MO, BY, 3 MO + 1, BX, the
//                                                                    Fq2 product's 15, and the last spread constant)
//   FQ28_SUB_SUB2_2_2 (3 -> 1)                                       sub_sub2<2, 2>
//   FQ28_MUL (2 -> 1), FQ28_SQR (1 -> 1)                             mul, sqr
//   FQ28_MUL_RAW_10 (3 -> 1)                                         mul(sub_raw<10>(a, b), c): the raw first operand as
//                                                                    madd / xadd form it
//   FQ28_MUL_SUB2_<B> (4 -> 1)                                       mul_sub2<B>(x0, y0, x1, y1)   B = 2 5
//   FQ28_CANON, FQ28_WRED (1 -> 1)                                   canon, fq28_wred
//   FQ28_IS_ZERO_FULL, FQ28_IS_ZERO_LAZY (1 -> 1 truth value)        is_zero_full, fq28_is_zero_lazy
//   FQ28_UNPACK, FQ28_IMPORT (12 words -> 1), FQ28_EXPORT (1 -> 12 words)
//   FQ2X_ADD (4 -> 2), FQ2X_SUB_B_<B> (4 -> 2), FQ2X_SUB_SUB2_2_2 (6 -> 2), FQ2X_MUL (4 -> 2)
//   FQ2X_SQR_B_<A> (2 -> 2)                                          sqr_b<A>   A = 2 4 5 6 8 10 13 and the static limit 30
//   FQ2X_IS_ZERO_FULL (2 -> 1 truth value)
//   FR_* / FQ32_*: ADD SUB (2 -> 1), NEG DBL SQR TO_MONT FROM_MONT (1 -> 1)     Fp<FrCfg>, Fp<FqCfg>
//   G1_MDBL (2 -> 4), G1_XDBL (4 -> 4), G1_MADD / G1_MADD_NEG (acc 4 + p 2 -> 4), G1_XADD (8 -> 4)     over Fq28
//   G2_*: the same with twice the slots                                                              over Fq2x
namespace zkdev {

ZK_DI Fq2x hk_q2(const Fq28* a) { return Fq2x{a[0], a[1]}; }
ZK_DI void hk_put(Fq28* o, const Fq28& v) { o[0] = v; }
ZK_DI void hk_put(Fq28* o, const Fq2x& v) {
    o[0] = v.c0;
    o[1] = v.c1;
}
ZK_DI void hk_put(Fq28* o, bool v) {
    o[0] = Fq28::zero();
    o[0].l[0] = v ? 1u : 0u;
}
template <class C>
ZK_DI Fp<C> hk_fp(const Fq28& s) {
    Fp<C> r;
#pragma unroll
    for (int i = 0; i < C::N; i++) r.l[i] = s.l[i];
    return r;
}
template <class C>
ZK_DI void hk_put(Fq28* o, const Fp<C>& v) {
    o[0] = Fq28::zero();
#pragma unroll
    for (int i = 0; i < C::N; i++) o[0].l[i] = v.l[i];
}
ZK_DI Fq28 hk_field(const Fq28* a, const Fq28*) { return a[0]; }
ZK_DI Fq2x hk_field(const Fq28* a, const Fq2x*) { return hk_q2(a); }
template <class F>
ZK_DI Affine<F> hk_aff(const Fq28* a) {
    constexpr int W = sizeof(F) / sizeof(Fq28);
    return Affine<F>{hk_field(a, (const F*)nullptr), hk_field(a + W, (const F*)nullptr)};
}
template <class F>
ZK_DI XYZZ<F> hk_pt(const Fq28* a) {
    constexpr int W = sizeof(F) / sizeof(Fq28);
    return XYZZ<F>{hk_field(a, (const F*)nullptr), hk_field(a + W, (const F*)nullptr), hk_field(a + 2 * W, (const F*)nullptr),
                   hk_field(a + 3 * W, (const F*)nullptr)};
}
template <class F>
ZK_DI void hk_put(Fq28* o, const XYZZ<F>& p) {
    constexpr int W = sizeof(F) / sizeof(Fq28);
    hk_put(o, p.x);
    hk_put(o + W, p.y);
    hk_put(o + 2 * W, p.zz);
    hk_put(o + 3 * W, p.zzz);
}
template <class F>
ZK_DI XYZZ<F> hk_madd(const Fq28* a, bool negate) {
    constexpr int W = sizeof(F) / sizeof(Fq28);
    XYZZ<F> acc = hk_pt<F>(a);
    madd(acc, hk_aff<F>(a + 4 * W), negate);
    return acc;
}
ZK_DI Fq28 hk_export(const Fq28& a) {
    Fq28 r = Fq28::zero();
    fq28_export(a, r.l);
    return r;
}

// X(name, slots in, slots out, the value written to the output slots): `a` is the array of input slots.
// tests/field_cases.py holds the same table in the same order.
#define ZK_HK_B(X, B)                                              \
    X(FQ28_SUB_B_##B, 2, 1, sub_b<B>(a[0], a[1]))                  \
    X(FQ28_NEG_B_##B, 1, 1, neg_b<B>(a[0]))                        \
    X(FQ28_SUB_RAW_##B, 2, 1, sub_raw<B>(a[0], a[1]))              \
    X(FQ28_NEG_RAW_##B, 1, 1, neg_raw<B>(a[0]))                    \
    X(FQ2X_SUB_B_##B, 4, 2, sub_b<B>(hk_q2(a), hk_q2(a + 2)))
#define ZK_HK_FP(X, P, C)                                          \
    X(P##_ADD, 2, 1, add(hk_fp<C>(a[0]), hk_fp<C>(a[1])))          \
    X(P##_SUB, 2, 1, sub(hk_fp<C>(a[0]), hk_fp<C>(a[1])))          \
    X(P##_NEG, 1, 1, neg(hk_fp<C>(a[0])))                          \
    X(P##_DBL, 1, 1, dbl(hk_fp<C>(a[0])))                          \
    X(P##_SQR, 1, 1, sqr(hk_fp<C>(a[0])))                          \
    X(P##_TO_MONT, 1, 1, to_mont(hk_fp<C>(a[0])))                  \
    X(P##_FROM_MONT, 1, 1, from_mont(hk_fp<C>(a[0])))
#define ZK_HK_GROUP(X, P, F, W)                                    \
    X(P##_MDBL, 2 * W, 4 * W, mdbl(hk_aff<F>(a)))                  \
    X(P##_XDBL, 4 * W, 4 * W, xdbl(hk_pt<F>(a)))                   \
    X(P##_MADD, 6 * W, 4 * W, hk_madd<F>(a, false))                \
    X(P##_MADD_NEG, 6 * W, 4 * W, hk_madd<F>(a, true))             \
    X(P##_XADD, 8 * W, 4 * W, xadd(hk_pt<F>(a), hk_pt<F>(a + 4 * W)))
#define ZK_HK_OPS(X)                                               \
    X(FQ28_ADD, 2, 1, add(a[0], a[1]))                             \
    X(FQ28_DBL, 1, 1, dbl(a[0]))                                   \
    ZK_HK_B(X, 2) ZK_HK_B(X, 4) ZK_HK_B(X, 5) ZK_HK_B(X, 7) ZK_HK_B(X, 10) ZK_HK_B(X, 15) ZK_HK_B(X, 63) \
    X(FQ28_SUB_SUB2_2_2, 3, 1, sub_sub2<2, 2>(a[0], a[1], a[2]))   \
    X(FQ28_MUL, 2, 1, mul(a[0], a[1]))                             \
    X(FQ28_SQR, 1, 1, sqr(a[0]))                                   \
    X(FQ28_MUL_RAW_10, 3, 1, mul(sub_raw<10>(a[0], a[1]), a[2]))   \
    X(FQ28_MUL_SUB2_2, 4, 1, mul_sub2<2>(a[0], a[1], a[2], a[3]))  \
    X(FQ28_MUL_SUB2_5, 4, 1, mul_sub2<5>(a[0], a[1], a[2], a[3]))  \
    X(FQ28_CANON, 1, 1, canon(a[0]))                               \
    X(FQ28_WRED, 1, 1, fq28_wred(a[0]))                            \
    X(FQ28_IS_ZERO_FULL, 1, 1, is_zero_full(a[0]))                 \
    X(FQ28_IS_ZERO_LAZY, 1, 1, fq28_is_zero_lazy(a[0]))            \
    X(FQ28_UNPACK, 1, 1, fq28_unpack(a[0].l))                      \
    X(FQ28_IMPORT, 1, 1, fq28_import(a[0].l))                      \
    X(FQ28_EXPORT, 1, 1, hk_export(a[0]))                          \
    X(FQ2X_ADD, 4, 2, add(hk_q2(a), hk_q2(a + 2)))                 \
    X(FQ2X_SUB_SUB2_2_2, 6, 2, sub_sub2<2, 2>(hk_q2(a), hk_q2(a + 2), hk_q2(a + 4))) \
    X(FQ2X_MUL, 4, 2, mul(hk_q2(a), hk_q2(a + 2)))                 \
    X(FQ2X_SQR_B_2, 2, 2, sqr_b<2>(hk_q2(a)))                      \
    X(FQ2X_SQR_B_4, 2, 2, sqr_b<4>(hk_q2(a)))                      \
    X(FQ2X_SQR_B_5, 2, 2, sqr_b<5>(hk_q2(a)))                      \
    X(FQ2X_SQR_B_6, 2, 2, sqr_b<6>(hk_q2(a)))                      \
    X(FQ2X_SQR_B_8, 2, 2, sqr_b<8>(hk_q2(a)))                      \
    X(FQ2X_SQR_B_10, 2, 2, sqr_b<10>(hk_q2(a)))                    \
    X(FQ2X_SQR_B_13, 2, 2, sqr_b<13>(hk_q2(a)))                    \
    X(FQ2X_SQR_B_30, 2, 2, sqr_b<30>(hk_q2(a)))                    \
    X(FQ2X_IS_ZERO_FULL, 2, 1, is_zero_full(hk_q2(a)))             \
    ZK_HK_FP(X, FR, FrCfg) ZK_HK_FP(X, FQ32, FqCfg)                \
    ZK_HK_GROUP(X, G1, Fq28, 1) ZK_HK_GROUP(X, G2, Fq2x, 2)

enum FieldOp : uint32_t {
#define X(name, ni, no, ...) FOP_##name,
    ZK_HK_OPS(X)
#undef X
    FOP_COUNT
};

template <uint32_t OP> struct FieldOpRun;
#define X(name, ni, no, ...)                                                          \
    template <> struct FieldOpRun<FOP_##name> {                                       \
        static constexpr int NI = ni, NO = no;                                        \
        static ZK_DI void run(const Fq28* a, Fq28* o) { hk_put(o, __VA_ARGS__); }     \
    };
ZK_HK_OPS(X)
#undef X

template <uint32_t OP>
__global__ void __launch_bounds__(64) k_field_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    constexpr int NI = FieldOpRun<OP>::NI, NO = FieldOpRun<OP>::NO;
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    Fq28 a[NI], o[NO];
#pragma unroll
    for (int s = 0; s < NI; s++)
#pragma unroll
        for (int j = 0; j < 14; j++) a[s].l[j] = in[((size_t)row * NI + s) * 16 + j];
    FieldOpRun<OP>::run(a, o);
#pragma unroll
    for (int s = 0; s < NO; s++)
#pragma unroll
        for (int j = 0; j < 16; j++) out[((size_t)row * NO + s) * 16 + j] = j < 14 ? o[s].l[j] : 0u;
}

// ---------------------------------------------------------------------------------------------------------------- rows
// The wave-cooperative layer (coop_field.h, coop_curve.h): ONE row of COOP_W threads applies one function to the limbs of
// its case, loaded with coop_load from the Fq28 slots as they are and stored with coop_store.  Blocks are four rows (the 64
// lanes of a GPU wave hold four different cases; a row count that is no multiple of 4 ends in a wave with one to three rows
// live), the row index is coop_row(), rows past n return before any row operation, truth values and word outputs are
// written by lane 0, and a row that needs the LDS scratch of coop_pow / inv gets the CoopPowTab of its place in the block.
//
//   op family (in -> out slots)                                      the function
//   COOP_FQ_ADD (2 -> 1), COOP_FQ_DBL (1 -> 1)                       add, dbl                                  over CFq
//   COOP_FQ_SUB_B_<B>, COOP_FQ_SUB_RAW_<B> (2 -> 1),                 sub_b<B>, sub_raw<B>, neg_b<B>, neg_raw<B>
//   COOP_FQ_NEG_B_<B>, COOP_FQ_NEG_RAW_<B> (1 -> 1)                  B = 2 4 5 7 8 9 10 14 15 16 18 32 35: every bound that
//                                                                    coop_curve.h, coop_tail.cpp, coop_verify.cpp and
//                                                                    coop_pairing.cpp instantiate, and 63
//   COOP_FQ_SUB_SUB2_2_2 (3 -> 1)                                    sub_sub2<2, 2>
//   COOP_FQ_MUL (2 -> 1), COOP_FQ_SQR (1 -> 1), COOP_FQ_MUL2 (4 -> 2)   mul, sqr, mul2(a0, b0, a1, b1)
//   COOP_FQ_MUL_SUB2_<B> (4 -> 1)                                    mul_sub2<B>(x0, y0, x1, y1)   B = 2 5
//   COOP_FQ_MUL_RAW_10 (3 -> 1)                                      mul(sub_raw<10>(a, b), c)
//   COOP_FQ_WNORM, COOP_FQ_EXACT (1 -> 1)                            coop_wnorm, coop_exact
//   COOP_FQ_IS_ZERO_NORM, COOP_FQ_IS_ZERO_FULL (1 -> 1 truth value)
//   COOP_PRODUCTS_<K>_<NT> (2 K NT -> K)                             coop_products<K, NT, MASK> with the term masks of the
//                                                                    group law: the x of accumulator k, term t in slot
//                                                                    k NT + t, its y in slot K NT + k NT + t, EVERY
//                                                                    accumulator written out
//   COOP_FQ2_ADD (4 -> 2), COOP_FQ2_SUB_B_<B> (4 -> 2), COOP_FQ2_SUB_SUB2_2_2 (6 -> 2), COOP_FQ2_MUL (4 -> 2)      over CFq2
//   COOP_FQ2_SQR_B_<A> (2 -> 2)                                      sqr_b<A>   A = 2 4 5 6 7 8 9 10 (coop_slot_sqr, sqr)
//   COOP_FQ2_IS_ZERO_NORM, COOP_FQ2_IS_ZERO_FULL (2 -> 1 truth value)
//   COOP_GATHER_SCATTER (1 -> 1)                                     coop_scatter(coop_gather(x))
//   COOP_UNPACK, COOP_IMPORT, COOP_IMPORT_PLAIN (12 words -> 1), COOP_EXPORT (1 -> 12 words)
//   COOP_POW (base, 12-word exponent -> 1), COOP_INV_FERMAT, COOP_INV (1 -> 1), COOP_LEX_LARGEST (1 -> 1 truth value)
//   COOP_G1_XDBL (4 -> 4), COOP_G1_XADD (8 -> 4), COOP_G1_MADD (acc 4 + p 2 -> 4), COOP_G1_XDBL_XADD (8 -> 4)
//   COOP_G2_XDBL (8 -> 8), COOP_G2_XADD (16 -> 8), COOP_G2_XDBL_XADD (16 -> 8)      xadd(xdbl(a), b) as coop_tail.cpp chains it
// (No madd over CFq2 and no negating madd: the product instantiates neither on rows.)
struct HkSlot {
    Fq28 f;
    uint32_t pad[2];
};
static_assert(sizeof(HkSlot) == 64, "a slot is 16 words");
template <int N> struct HkRows { CFq v[N]; };
struct HkWords { uint32_t w[12]; };

ZK_DI CFq hc(const HkSlot& s) { return coop_load(s.f); }
ZK_DI CFq2 hc2(const HkSlot* s) { return CFq2{hc(s[0]), hc(s[1])}; }
ZK_DI CFq hc_field(const HkSlot* s, const CFq*) { return hc(s[0]); }
ZK_DI CFq2 hc_field(const HkSlot* s, const CFq2*) { return hc2(s); }
template <class F> ZK_DI XYZZ<F> hc_pt(const HkSlot* s) {
    constexpr int W = sizeof(F) / sizeof(CFq);
    return XYZZ<F>{hc_field(s, (const F*)nullptr), hc_field(s + W, (const F*)nullptr), hc_field(s + 2 * W, (const F*)nullptr),
                   hc_field(s + 3 * W, (const F*)nullptr)};
}
// the two pad words of a slot: zero on output, written by the two lanes that hold no limb
ZK_DI void hc_pad(HkSlot* o) {
#ifndef ZK_EMU
    if (coop_lane() >= 14) o->pad[coop_lane() - 14] = 0u;
#else
    o->pad[0] = o->pad[1] = 0u;
#endif
}
ZK_DI void hc_put(HkSlot* o, const CFq& v) {
    coop_store(o->f, v);
    hc_pad(o);
}
ZK_DI void hc_put(HkSlot* o, const CFq2& v) {
    hc_put(o, v.c0);
    hc_put(o + 1, v.c1);
}
template <int N> ZK_DI void hc_put(HkSlot* o, const HkRows<N>& v) {
#pragma unroll
    for (int k = 0; k < N; k++) hc_put(o + k, v.v[k]);
}
template <class F> ZK_DI void hc_put(HkSlot* o, const XYZZ<F>& p) {
    constexpr int W = sizeof(F) / sizeof(CFq);
    hc_put(o, p.x);
    hc_put(o + W, p.y);
    hc_put(o + 2 * W, p.zz);
    hc_put(o + 3 * W, p.zzz);
}
ZK_DI void hc_put(HkSlot* o, const HkWords& v) {   // (lane 0)
#ifndef ZK_EMU
    if (coop_lane() != 0) return;
#endif
    uint32_t* w = reinterpret_cast<uint32_t*>(o);   // the slot's 16 words
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = i < 12 ? v.w[i] : 0u;
}
ZK_DI void hc_put(HkSlot* o, bool v) {
    HkWords w = {};
    w.w[0] = v ? 1u : 0u;
    hc_put(o, w);
}
ZK_DI CFq2 hc_mul2(const HkSlot* a) {
    CFq2 r;
    mul2(hc(a[0]), hc(a[1]), hc(a[2]), hc(a[3]), r.c0, r.c1);
    return r;
}
template <int K, int NT, uint64_t MASK> ZK_DI HkRows<K> hc_products(const HkSlot* a) {
    CLanes x[K][NT], y[K][NT];
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            x[k][t] = hc(a[k * NT + t]).l;
            y[k][t] = hc(a[K * NT + k * NT + t]).l;
        }
    HkRows<K> r;
    coop_products<K, NT, MASK>(x, y, r.v);
    return r;
}
ZK_DI HkWords hc_export(const CFq& a) {
    HkWords r = {};
    coop_export(a, r.w);
    return r;
}
ZK_DI CFq hc_pow(const HkSlot* a, CoopPowTab& tab) {
    uint32_t e[12];
#pragma unroll
    for (int i = 0; i < 12; i++) e[i] = a[1].f.l[i];
    return coop_pow(hc(a[0]), e, tab);
}
ZK_DI XYZZ<CFq> hc_madd(const HkSlot* a) {
    XYZZ<CFq> acc = hc_pt<CFq>(a);
    madd(acc, Affine<CFq>{hc(a[4]), hc(a[5])});
    return acc;
}

// X(name, slots in, slots out, the value written to the output slots): `a` is the row's input slots, `tab` its LDS scratch.
// tests/coop_cases.py holds the same table in the same order.
#define ZK_HK_CB(X, B)                                                          \
    X(COOP_FQ_SUB_B_##B, 2, 1, sub_b<B>(hc(a[0]), hc(a[1])))                    \
    X(COOP_FQ_NEG_B_##B, 1, 1, neg_b<B>(hc(a[0])))                              \
    X(COOP_FQ_SUB_RAW_##B, 2, 1, sub_raw<B>(hc(a[0]), hc(a[1])))                \
    X(COOP_FQ_NEG_RAW_##B, 1, 1, neg_raw<B>(hc(a[0])))                          \
    X(COOP_FQ2_SUB_B_##B, 4, 2, sub_b<B>(hc2(a), hc2(a + 2)))
#define ZK_HK_CGROUP(X, P, F, W)                                                \
    X(P##_XDBL, 4 * W, 4 * W, xdbl(hc_pt<F>(a)))                                \
    X(P##_XADD, 8 * W, 4 * W, xadd(hc_pt<F>(a), hc_pt<F>(a + 4 * W)))           \
    X(P##_XDBL_XADD, 8 * W, 4 * W, xadd(xdbl(hc_pt<F>(a)), hc_pt<F>(a + 4 * W)))
#define ZK_HK_COOP_OPS(X)                                                       \
    X(COOP_FQ_ADD, 2, 1, add(hc(a[0]), hc(a[1])))                               \
    X(COOP_FQ_DBL, 1, 1, dbl(hc(a[0])))                                         \
    ZK_HK_CB(X, 2) ZK_HK_CB(X, 4) ZK_HK_CB(X, 5) ZK_HK_CB(X, 7) ZK_HK_CB(X, 8) ZK_HK_CB(X, 9) ZK_HK_CB(X, 10) \
    ZK_HK_CB(X, 14) ZK_HK_CB(X, 15) ZK_HK_CB(X, 16) ZK_HK_CB(X, 18) ZK_HK_CB(X, 32) ZK_HK_CB(X, 35) ZK_HK_CB(X, 63) \
    X(COOP_FQ_SUB_SUB2_2_2, 3, 1, sub_sub2<2, 2>(hc(a[0]), hc(a[1]), hc(a[2]))) \
    X(COOP_FQ_MUL, 2, 1, mul(hc(a[0]), hc(a[1])))                               \
    X(COOP_FQ_SQR, 1, 1, sqr(hc(a[0])))                                         \
    X(COOP_FQ_MUL2, 4, 2, hc_mul2(a))                                           \
    X(COOP_FQ_MUL_SUB2_2, 4, 1, mul_sub2<2>(hc(a[0]), hc(a[1]), hc(a[2]), hc(a[3]))) \
    X(COOP_FQ_MUL_SUB2_5, 4, 1, mul_sub2<5>(hc(a[0]), hc(a[1]), hc(a[2]), hc(a[3]))) \
    X(COOP_FQ_MUL_RAW_10, 3, 1, mul(sub_raw<10>(hc(a[0]), hc(a[1])), hc(a[2]))) \
    X(COOP_FQ_WNORM, 1, 1, coop_wnorm(hc(a[0])))                                \
    X(COOP_FQ_EXACT, 1, 1, coop_exact(hc(a[0])))                                \
    X(COOP_FQ_IS_ZERO_NORM, 1, 1, hc(a[0]).is_zero_norm())                      \
    X(COOP_FQ_IS_ZERO_FULL, 1, 1, is_zero_full(hc(a[0])))                       \
    X(COOP_PRODUCTS_3_2, 12, 3, (hc_products<3, 2, 0b010111>(a)))               \
    X(COOP_PRODUCTS_2_2, 8, 2, (hc_products<2, 2, 0b0111>(a)))                  \
    X(COOP_PRODUCTS_6_1, 12, 6, (hc_products<6, 1, ~0ull>(a)))                  \
    X(COOP_PRODUCTS_6_2, 24, 6, (hc_products<6, 2, 0b010111111111>(a)))         \
    X(COOP_PRODUCTS_8_2, 32, 8, (hc_products<8, 2, ~0ull>(a)))                  \
    X(COOP_PRODUCTS_12_2, 48, 12, (hc_products<12, 2, ~0ull>(a)))               \
    X(COOP_FQ2_ADD, 4, 2, add(hc2(a), hc2(a + 2)))                              \
    X(COOP_FQ2_SUB_SUB2_2_2, 6, 2, sub_sub2<2, 2>(hc2(a), hc2(a + 2), hc2(a + 4))) \
    X(COOP_FQ2_MUL, 4, 2, mul(hc2(a), hc2(a + 2)))                              \
    X(COOP_FQ2_SQR_B_2, 2, 2, sqr_b<2>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_4, 2, 2, sqr_b<4>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_5, 2, 2, sqr_b<5>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_6, 2, 2, sqr_b<6>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_7, 2, 2, sqr_b<7>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_8, 2, 2, sqr_b<8>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_9, 2, 2, sqr_b<9>(hc2(a)))                                 \
    X(COOP_FQ2_SQR_B_10, 2, 2, sqr_b<10>(hc2(a)))                               \
    X(COOP_FQ2_IS_ZERO_NORM, 2, 1, hc2(a).is_zero_norm())                       \
    X(COOP_FQ2_IS_ZERO_FULL, 2, 1, is_zero_full(hc2(a)))                        \
    X(COOP_GATHER_SCATTER, 1, 1, coop_scatter(coop_gather(hc(a[0]))))           \
    X(COOP_UNPACK, 1, 1, coop_unpack(a[0].f.l))                                 \
    X(COOP_IMPORT, 1, 1, coop_import(a[0].f.l))                                 \
    X(COOP_IMPORT_PLAIN, 1, 1, coop_import_plain(a[0].f.l))                     \
    X(COOP_EXPORT, 1, 1, hc_export(hc(a[0])))                                   \
    X(COOP_POW, 2, 1, hc_pow(a, tab))                                           \
    X(COOP_INV_FERMAT, 1, 1, inv_fermat(hc(a[0]), tab))                         \
    X(COOP_INV, 1, 1, inv(hc(a[0]), tab))                                       \
    X(COOP_LEX_LARGEST, 1, 1, coop_lex_largest(hc(a[0])))                       \
    ZK_HK_CGROUP(X, COOP_G1, CFq, 1)                                            \
    X(COOP_G1_MADD, 6, 4, hc_madd(a))                                           \
    ZK_HK_CGROUP(X, COOP_G2, CFq2, 2)

enum CoopFieldOp : uint32_t {
    FOP_COOP_FIRST = FOP_COUNT - 1,      // (the row ops continue the codes of FieldOp)
#define X(name, ni, no, ...) FOP_##name,
    ZK_HK_COOP_OPS(X)
#undef X
    FOP_ALL_COUNT
};

template <uint32_t OP> struct CoopOpRun;
#define X(name, ni, no, ...)                                                                              \
    template <> struct CoopOpRun<FOP_##name> {                                                            \
        static constexpr int NI = ni, NO = no;                                                            \
        static ZK_DI void run(const HkSlot* a, HkSlot* o, CoopPowTab& tab) { hc_put(o, __VA_ARGS__); }    \
    };
ZK_HK_COOP_OPS(X)
#undef X

constexpr int HK_COOP_ROWS = 4;   // rows per block: the four rows of a GPU wave
template <uint32_t OP>
__global__ void __launch_bounds__(HK_COOP_ROWS * COOP_W) k_coop_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    ZK_SHARED CoopPowTab powtab[HK_COOP_ROWS];
    const uint32_t row = coop_row();
    if (row >= n) return;
    CoopOpRun<OP>::run((const HkSlot*)in + (size_t)row * CoopOpRun<OP>::NI, (HkSlot*)out + (size_t)row * CoopOpRun<OP>::NO,
                       powtab[coop_row_in_block()]);
}

}  // namespace zkdev

using namespace zkrt;

extern "C" zk_status zk_hook_field_op(uint32_t op, const uint32_t* in, uint32_t* out, size_t n) try {
    static const uint32_t slots[][2] = {
#define X(name, ni, no, ...) {ni, no},
        ZK_HK_OPS(X) ZK_HK_COOP_OPS(X)
#undef X
    };
    static_assert(sizeof(slots) / sizeof(slots[0]) == zkdev::FOP_ALL_COUNT, "one entry of the slot table per op");
    if (op >= zkdev::FOP_ALL_COUNT) return fail(ZK_ERR_INVALID_ARGUMENT, "unknown field op");
    if (!in || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    if (n > (1u << 20)) return fail(ZK_ERR_INVALID_ARGUMENT, "too many rows");
    const size_t in_bytes = n * slots[op][0] * 64, out_bytes = n * slots[op][1] * 64;
    ZK_TRY(use_device(0));
    DevBuf a, b;
    a.is_public = b.is_public = true;
    ZK_TRY(a.ensure(in_bytes));
    ZK_TRY(b.ensure(out_bytes));
    HIP_TRY(hipMemcpy(a.p, in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b.p, 0xa5, out_bytes));   // (a word no thread writes is not mistaken for a result)
    const dim3 grid((unsigned)((n + 63) / 64)), cgrid((unsigned)((n + zkdev::HK_COOP_ROWS - 1) / zkdev::HK_COOP_ROWS));
    switch (op) {
#define X(name, ni, no, ...)                                                                                                     \
    case zkdev::FOP_##name:                                                                                                      \
        ZK_LAUNCH(zkdev::k_field_op<zkdev::FOP_##name>, grid, dim3(64), 0, g_stream, a.as<uint32_t>(), b.as<uint32_t>(), (uint32_t)n); \
        break;
        ZK_HK_OPS(X)
#undef X
#define X(name, ni, no, ...)                                                                                                     \
    case zkdev::FOP_##name:                                                                                                      \
        ZK_LAUNCH(zkdev::k_coop_op<zkdev::FOP_##name>, cgrid, dim3(zkdev::HK_COOP_ROWS * zkdev::COOP_W), 0, g_stream, a.as<uint32_t>(), \
                  b.as<uint32_t>(), (uint32_t)n);                                                                                \
        break;
        ZK_HK_COOP_OPS(X)
#undef X
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(out, b.p, out_bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH
#endif
