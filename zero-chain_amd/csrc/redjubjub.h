// RedJubjub (core/jubjub/src/redjubjub.rs): signing with the re-randomised key the derive / gen_proof entries hand out, and
// the runtime's per-extrinsic signature check (core/primitives/src/signature.rs:65-82) for a batch, one verdict per signature.
// Included by wallet.cpp below its helpers (FS_MOD, fs_lt_mod, fs_to_uniform, jubjub_fixed_mul, jubjub_encode, WipeOnExit).
//
//   H*(a || b)   BLAKE2b-512 personalised "Zcash_RedJubjubH" over a then b, Fs::to_uniform          redjubjub.rs:24-26, util.rs:5-11
//   sign         r = H*(T || M), Rbar = write(r G), S = r + H*(Rbar || M) rsk                        redjubjub.rs:73-103
//   verify       vk, R = Point::read (no prime-order test), S < s, [8]([c]vk + R - [S]G) == O       redjubjub.rs:127-155
// G is FixedGenerators::Diversifier of the reference's signing calls, the generator of zkwit::tables().
//
// Signing runs on the host alone, and the secrets stay off the device.  Its control flow and table addresses do not depend on
// rsk, T or r: jubjub_fixed_mul picks by masks, and the Fs arithmetic on them below (fs_reduce_ct, fs_add_ct) subtracts the
// modulus under a mask.  What remains variable-time is the final conditional subtraction inside the host Fr routines under
// jubjub_fixed_mul, as wallet.cpp says of every secret scalar multiplication of this library.
// Verification has two forms, the same bytes:
//   host    zkwit::decode_point twice and a variable-time joint double-and-add, on the zk_set_host_threads pool
//   device  two launches, one wave per block.  The host hashes c_i = H*(Rbar_i || M_i) while the first runs; messages never
//           travel (variable length, and BLAKE2b is cheap beside the point work).
//     k_rj_decode   2n lanes, vk_i and R_i side by side: jubjub_dev.h read_point, k_into_xy's chain without [s]P - about 620
//                   dependent Fr products (~330 the inversion, ~290 the square root's exponentiation; Tonelli-Shanks adds up
//                   to 500 for the few x^2 of high 2-adic order).  LDS: the 16-slot window table, 32 768 B.
//     k_rj_check    n lanes, ONE joint chain [c]vk + [S](-G), then + R, three doublings, X == 0 && Y == Z - about 2 900
//                   dependent products:
//                     252 doublings, shared by both scalars (dbl-2008-hwcd: 8 products)                        2 016
//                     85 additions of a multiple of vk (1 .. 4 times vk cached as (Y + X, Y - X, 2dT, 2Z): 7)    595
//                     43 additions of a multiple of G (1 .. 32 times G, affine, from a table in memory: 6)       258
//                     the four cached multiples, R, the last three doublings                                      ~60
//                   The digits are signed FIXED windows (Booth: 3 bits for c, 6 for S, read off the scalar's bits per lane
//                   at run time - total for every value below 2^252, which every c and S below s is), not a width-w
//                   NAF: a NAF puts each lane's additions at its own positions, and a wave then walks through an addition
//                   at nearly every one of the 252 positions (5 500 products); with fixed windows all 64 lanes add at the
//                   same 85 + 43.  LDS, [slot][word][lane] as jubjub_dev.h Lds: 16 slots of cached multiples and 2 slots for
//                   the words of c and S (dynamic indexing of registers would go to scratch) = 18 x 32 x 64 = 36 864 B.
// The inputs are public: nothing in verification is constant-time, and its buffers are freed without the wipe.
#pragma once
#include "jubjub_dev.h"   // (not xt_inputs.h: that header holds k_into_xy, which this unit must not compile a copy of)
#include "host_common.h"
#include "host_math.h"
#include "transfer_witness.h"
#include "blake2s.h"

namespace zkrj {

using zkdev::Fr;
using zkrt::fail;
using zkxt::EP;
using zkxt::Lds;

enum { RJ_OK = 0, RJ_BAD_VK = 1, RJ_BAD_R = 2, RJ_BAD_S = 3, RJ_BAD_EQUATION = 4 };
// ZKAMD_REDJUBJUB_HOST_MAX: signatures up to which the host form runs.  Measured crossover (profiles/r11_redjubjub_probe.json, 16 host
// threads): the two kernels are 3.0 ms whatever the batch holds, the host form 2.38 ms at 256 signatures and 8.23 ms at 1024 - the
// lines cross at 338, rounded down to a multiple of 64.
constexpr size_t HOST_MAX = 320;
constexpr uint32_t DECODE_LDS_BYTES = 16 * 32 * 64, CHECK_LDS_SLOTS = 18, CHECK_LDS_BYTES = CHECK_LDS_SLOTS * 32 * 64;
constexpr int VK_WINDOW = 3, G_WINDOW = 6, G_MULTIPLES = 1 << (G_WINDOW - 1);
constexpr uint32_t GTAB_WORDS = 8 + G_MULTIPLES * 24;   // 2d | per multiple: y + x, y - x, 2 d x y (Montgomery)
static_assert(G_WINDOW == 2 * VK_WINDOW && 252 % G_WINDOW == 0, "a G window every second vk window, the last at bit 252");

ZK_DI Fr ld_fr(const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 lo = q[0], hi = q[1];
    Fr r;
    r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
    r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
    return r;
}

// enc: m x 8 words.  xy: m x 16 words, x then y in Montgomery form (zero where refused).  status: m words, zkxt::INTO_XY_*.
static __global__ void __launch_bounds__(64)
k_rj_decode(const uint32_t* enc, uint32_t* xy, uint32_t* status, uint32_t m) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= m) return;
    const Lds L{table + threadIdx.x};
    Fr x = Fr::zero(), y, xm = Fr::zero(), ym, d;
    const uint32_t st = zkxt::read_point(L, enc + (size_t)t * 8, &x, &y, &xm, &ym, &d);
    if (st != zkxt::INTO_XY_OK) xm = ym = Fr::zero();
    uint4* o = reinterpret_cast<uint4*>(xy + (size_t)t * 16);
    o[0] = make_uint4(xm.l[0], xm.l[1], xm.l[2], xm.l[3]);
    o[1] = make_uint4(xm.l[4], xm.l[5], xm.l[6], xm.l[7]);
    o[2] = make_uint4(ym.l[0], ym.l[1], ym.l[2], ym.l[3]);
    o[3] = make_uint4(ym.l[4], ym.l[5], ym.l[6], ym.l[7]);
    status[t] = st;
}

// The signed digit of the W-bit window at bit `pos` of the scalar whose 8 plain words lie in `slot`:
// -2^(W-1) b[pos+W-1] + sum_{k < W-1} 2^k b[pos+k] + b[pos-1], in -2^(W-1) .. 2^(W-1); the digits of the windows at
// 0, W, 2W .. 252 sum to the scalar when it is below 2^252 (the window at 252 then holds b[251] alone).  `pos` is the same
// in every lane.
template <int W>
ZK_DI int booth_digit(const Lds& L, uint32_t slot, uint32_t pos) {
    uint32_t v;
    if (pos == 0) {
        v = L.base[slot * 8 * 64] << 1;
    } else {
        const uint32_t p = pos - 1, wi = p >> 5;
        const uint32_t lo = L.base[(slot * 8 + wi) * 64], hi = wi < 7 ? L.base[(slot * 8 + wi + 1) * 64] : 0u;
        v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31));
    }
    v &= (2u << W) - 1;
    return (int)((v >> 1) & ((1u << (W - 1)) - 1)) + (int)(v & 1u) - (int)((v >> W) << (W - 1));
}
// p + sign * (an affine point as y + x, y - x, 2 d x y): ext_add_cached with Z = 1, one product less
ZK_DI EP ext_add_affine(const EP& p, const Fr& q_ypx, const Fr& q_ymx, const Fr& q_td2, bool negative, bool want_t) {
    const Fr a = mul(sub(p.Y, p.X), negative ? q_ypx : q_ymx), b = mul(add(p.Y, p.X), negative ? q_ymx : q_ypx);
    const Fr c = mul(p.T, q_td2), d = dbl(p.Z);
    const Fr e = sub(b, a), h = add(b, a);
    const Fr f = negative ? add(d, c) : sub(d, c), g = negative ? sub(d, c) : add(d, c);
    EP r;
    r.X = mul(e, f);
    r.Y = mul(g, h);
    r.Z = mul(f, g);
    r.T = want_t ? mul(e, h) : Fr::zero();
    return r;
}

// gtab: GTAB_WORDS (gtable()).  xy, status: k_rj_decode's, vk_i at 2i and R_i at 2i + 1.  cs: n x 16 words, c_i then S_i, plain.
// reason: n words, RJ_*.
static __global__ void __launch_bounds__(64)
k_rj_check(const uint32_t* gtab, const uint32_t* xy, const uint32_t* status, const uint32_t* cs, uint32_t* reason, uint32_t n) {
    ZK_SHARED uint32_t table[CHECK_LDS_SLOTS * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Lds L{table + threadIdx.x};
    const Fr s_plain = ld_fr(cs + (size_t)t * 16 + 8);
    uint32_t why = RJ_OK;
    {
        const uint64_t fs[4] = ZK_JUBJUB_FS_MODULUS_64;
        uint32_t bo = 0, co;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            (void)__builtin_subc(s_plain.l[i], (uint32_t)(fs[i >> 1] >> (32 * (i & 1))), bo, &co);
            bo = co;
        }
        if (bo == 0) why = RJ_BAD_S;   // S - s does not borrow: S >= s
    }
    if (status[2 * (size_t)t + 1] != zkxt::INTO_XY_OK) why = RJ_BAD_R;
    if (status[2 * (size_t)t] != zkxt::INTO_XY_OK) why = RJ_BAD_VK;   // the reference reads the key first
    if (why == RJ_OK) {
        enum { SLOT_C = 16, SLOT_S = 17 };
        L.st(SLOT_C, ld_fr(cs + (size_t)t * 16));
        L.st(SLOT_S, s_plain);
        const Fr d2 = ld_fr(gtab);
        {   // vk, 2 vk, 3 vk, 4 vk in slots 4 i .. 4 i + 3
            const Fr x = ld_fr(xy + (size_t)t * 32), y = ld_fr(xy + (size_t)t * 32 + 8);
            EP q{x, y, Fr::one(), mul(x, y)};
            zkxt::cache_put(L, 0, q, d2);
            q = zkxt::ext_dbl(q, true);
            zkxt::cache_put(L, 1, q, d2);
#pragma unroll 1
            for (uint32_t i = 2; i < 4; i++) {
                q = zkxt::ext_add_cached(L, q, 0, false, true);
                zkxt::cache_put(L, i, q, d2);
            }
        }
        EP acc = zkxt::ep_neutral();
#pragma unroll 1
        for (int j = 252 / VK_WINDOW; j >= 0; j--) {
            if (j != 252 / VK_WINDOW) {
                acc = zkxt::ext_dbl(acc, false);
                acc = zkxt::ext_dbl(acc, false);
                acc = zkxt::ext_dbl(acc, true);
            }
            const int dv = booth_digit<VK_WINDOW>(L, SLOT_C, (uint32_t)(VK_WINDOW * j));
            if (dv) acc = zkxt::ext_add_cached(L, acc, (uint32_t)((dv < 0 ? -dv : dv) - 1), dv < 0, true);
            if (!(j & 1)) {
                const int dg = booth_digit<G_WINDOW>(L, SLOT_S, (uint32_t)(VK_WINDOW * j));
                if (dg) {   // - [S]G: the digit's sign turned round
                    const uint32_t* e = gtab + 8 + (size_t)((dg < 0 ? -dg : dg) - 1) * 24;
                    acc = ext_add_affine(acc, ld_fr(e), ld_fr(e + 8), ld_fr(e + 16), dg > 0, j == 0);
                }
            }
        }
        {   // + R, the cofactor, the neutral element
            const Fr x = ld_fr(xy + (size_t)t * 32 + 16), y = ld_fr(xy + (size_t)t * 32 + 24);
            acc = ext_add_affine(acc, add(y, x), sub(y, x), mul(mul(x, y), d2), false, false);
            acc = zkxt::ext_dbl(zkxt::ext_dbl(zkxt::ext_dbl(acc, false), false), false);
            if (!(acc.X.is_zero() && acc.Y == acc.Z)) why = RJ_BAD_EQUATION;
        }
    }
    reason[t] = why;
}

// ---- host side
// d2 and the multiples 1 .. G_MULTIPLES of G as the kernel reads them, built once per process
inline const std::vector<uint32_t>& gtable() {
    static const std::vector<uint32_t> tab = [] {
        const zkwit::JPoint g = zkwit::tables().win[0][1];
        std::vector<zkwit::EPoint> proj(G_MULTIPLES);
        proj[0] = zkwit::to_ext(g);
        for (int i = 1; i < G_MULTIPLES; i++) proj[i] = zkwit::ext_add(proj[i - 1], proj[0]);
        std::vector<zkwit::JPoint> aff(G_MULTIPLES);
        zkwit::batch_to_affine(proj.data(), aff.data(), G_MULTIPLES);
        std::vector<uint32_t> w(GTAB_WORDS);
        const zkhost::Fr d2 = zkwit::edwards_d().dbl();
        static_assert(sizeof(zkhost::Fr) == 32, "four 64-bit limbs: the kernels' eight words");
        memcpy(&w[0], d2.l, 32);
        for (int i = 0; i < G_MULTIPLES; i++) {
            const zkhost::Fr e[3] = {aff[i].y + aff[i].x, aff[i].y - aff[i].x, aff[i].x * aff[i].y * d2};
            memcpy(&w[8 + 24 * i], e, 96);
        }
        return w;
    }();
    return tab;
}

constexpr uint8_t H_STAR_PERSON[16] = {'Z', 'c', 'a', 's', 'h', '_', 'R', 'e', 'd', 'J', 'u', 'b', 'j', 'u', 'b', 'H'};
inline void h_star(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint64_t out[4]) {
    zkhash::Blake2b h(H_STAR_PERSON);
    h.update(a, a_len);
    h.update(b, b_len);
    uint8_t d[64];
    h.finish(d);
    fs_to_uniform(d, 64, out);
}
// ---- Fs on secrets: no branch and no early exit on a value derived from rsk or r
// v mod s for v < 2 s: v - s is taken, and kept under a mask when it does not borrow
inline void fs_reduce_ct(uint64_t v[4]) {
    uint64_t d[4];
    zkhost::u128 bo = 0;
    for (int i = 0; i < 4; i++) {
        const zkhost::u128 t = (zkhost::u128)v[i] - FS_MOD[i] - bo;
        d[i] = (uint64_t)t;
        bo = (t >> 64) & 1;
    }
    const uint64_t keep = (uint64_t)bo - 1;   // all-ones: no borrow, v >= s
    for (int i = 0; i < 4; i++) v[i] = (d[i] & keep) | (v[i] & ~keep);
    explicit_bzero(d, sizeof(d));
}
// v < s ?  by the borrow of v - s
inline bool fs_lt_mod_ct(const uint64_t v[4]) {
    zkhost::u128 bo = 0;
    for (int i = 0; i < 4; i++) bo = (((zkhost::u128)v[i] - FS_MOD[i] - bo) >> 64) & 1;
    return bo != 0;
}
// (a + b) mod s for a, b < s (s < 2^252: no carry out of 256 bits); out may be a or b
inline void fs_add_ct(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    zkhost::u128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (zkhost::u128)a[i] + b[i];
        out[i] = (uint64_t)c;
        c >>= 64;
    }
    fs_reduce_ct(out);
}
// Fs::to_uniform of a 64-byte digest, bit by bit as wallet.cpp's fs_to_uniform
inline void fs_to_uniform_ct(const uint8_t le[64], uint64_t out[4]) {
    uint64_t v[4] = {0, 0, 0, 0};
    WipeOnExit wipe_v{v, sizeof(v)};
    for (size_t i = 64; i-- > 0;)
        for (int b = 7; b >= 0; b--) {
            for (int k = 3; k > 0; k--) v[k] = (v[k] << 1) | (v[k - 1] >> 63);
            v[0] = (v[0] << 1) | ((le[i] >> b) & 1u);
            fs_reduce_ct(v);
        }
    memcpy(out, v, 32);
}
// a b mod s for a PUBLIC a < 2^252 (the loop branches on ITS bits only) and a secret b < s
inline void fs_mul_public(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    uint64_t acc[4] = {0, 0, 0, 0};
    WipeOnExit wipe_acc{acc, sizeof(acc)};
    for (int bit = 251; bit >= 0; bit--) {
        fs_add_ct(acc, acc, acc);
        if ((a[bit >> 6] >> (bit & 63)) & 1) fs_add_ct(acc, b, acc);
    }
    memcpy(out, acc, 32);
}

inline zk_status check_offsets(size_t n, const uint8_t* msgs, const uint64_t* offs) {
    for (size_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i]) return fail(ZK_ERR_INVALID_ARGUMENT, "msg_offsets decrease at message " + std::to_string(i));
    if (!msgs && offs[n] != offs[0]) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return ZK_OK;
}

// PrivateKey::sign for n keys, the 80 bytes T of each from the caller
inline zk_status sign(size_t n, const uint8_t* rsk, const uint8_t* t80, const uint8_t* msgs, const uint64_t* offs, uint8_t* sigs_out) {
    ZK_TRY(check_offsets(n, msgs, offs));
    (void)zkwit::tables();
    return zkrt::for_each_status(n, 64, [&](size_t i) -> zk_status {
        uint64_t sk[4], r[4], c[4], cs[4], s[4];
        uint8_t digest[64];
        zkhash::Blake2b h(H_STAR_PERSON);   // of r = H*(T || M): its state is a secret's
        WipeOnExit wipe_sk{sk, sizeof(sk)}, wipe_r{r, sizeof(r)}, wipe_cs{cs, sizeof(cs)}, wipe_d{digest, sizeof(digest)}, wipe_h{&h, sizeof(h)};
        zkrt::load_scalar_le(rsk + 32 * i, sk);
        if (!fs_lt_mod_ct(sk)) return fail(ZK_ERR_INVALID_ARGUMENT, "rsk " + std::to_string(i) + " is not a canonical Fs scalar");
        const uint8_t* m = msgs ? msgs + offs[i] : nullptr;
        const size_t m_len = (size_t)(offs[i + 1] - offs[i]);
        h.update(t80 + 80 * i, 80);
        h.update(m, m_len);
        h.finish(digest);
        fs_to_uniform_ct(digest, r);
        const zkwit::JPoint rg = jubjub_fixed_mul(r);
        uint8_t* sig = sigs_out + 64 * i;
        jubjub_encode(rg.x, rg.y, sig);
        h_star(sig, 32, m, m_len, c);
        fs_mul_public(c, sk, cs);
        fs_add_ct(cs, r, s);
        memcpy(sig + 32, s, 32);
        return ZK_OK;
    });
}

// PublicKey::verify of one signature, c = H*(Rbar || M) given
inline uint8_t verify_one(const uint8_t vk[32], const uint8_t sig[64], const uint64_t c[4]) {
    zkwit::JPoint key, r;
    if (!zkwit::decode_point(vk, &key)) return RJ_BAD_VK;
    if (!zkwit::decode_point(sig, &r)) return RJ_BAD_R;
    uint64_t s[4];
    zkrt::load_scalar_le(sig + 32, s);
    if (!fs_lt_mod(s)) return RJ_BAD_S;
    auto dbl = [](const zkwit::EPoint& p) {   // dbl-2008-hwcd, a = -1
        const zkhost::Fr a = p.X.sqr(), b = p.Y.sqr(), cc = p.Z.sqr().dbl();
        const zkhost::Fr d = zkhost::Fr::zero() - a;
        const zkhost::Fr e = (p.X + p.Y).sqr() - a - b, g = d + b, f = g - cc, h = d - b;
        return zkwit::EPoint{e * f, g * h, f * g, e * h};
    };
    // [c]vk + [S](-G): one chain of doublings, the addend picked by the two bits
    const zkwit::JPoint g = zkwit::tables().win[0][1];
    zkwit::EPoint add[4];
    add[1] = zkwit::to_ext(key);
    add[2] = zkwit::to_ext(zkwit::JPoint{zkhost::Fr::zero() - g.x, g.y});
    add[3] = zkwit::ext_add(add[1], add[2]);
    zkwit::EPoint acc = zkwit::ext_zero();
    for (int bit = 251; bit >= 0; bit--) {
        acc = dbl(acc);
        const unsigned k = (unsigned)((c[bit >> 6] >> (bit & 63)) & 1) | (unsigned)(((s[bit >> 6] >> (bit & 63)) & 1) << 1);
        if (k) acc = zkwit::ext_add(acc, add[k]);
    }
    acc = dbl(dbl(dbl(zkwit::ext_add(acc, zkwit::to_ext(r)))));
    return acc.X.is_zero() && acc.Y == acc.Z ? RJ_OK : RJ_BAD_EQUATION;
}

// n signatures (zk_redjubjub_verify_batch).  device < 0, or n <= ZKAMD_REDJUBJUB_HOST_MAX (read per call; 0 = always the
// device form): the host form.  Else the two kernels on the library stream of `device`.
inline zk_status verify_batch(size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* offs, int device,
                              uint8_t* ok_out, uint8_t* reason_out) {
    ZK_TRY(check_offsets(n, msgs, offs));
    const char* e = getenv("ZKAMD_REDJUBJUB_HOST_MAX");
    const size_t host_max = e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
    const bool on_host = device < 0 || n <= host_max;
    (void)zkwit::tables();
    // c_i = H*(Rbar_i || M_i) of signatures [first, first + np) into cs (np x 64 bytes: c_i, S_i), or straight to the verdicts
    std::vector<uint8_t> cs;
    auto hash_range = [&](size_t first, size_t np) {
        const unsigned nth = zkrt::host_threads(np, 64);
        auto work = [&](unsigned th) {
            for (size_t i = first + np * th / nth; i < first + np * (th + 1) / nth; i++) {
                uint64_t c[4];
                h_star(sigs + 64 * i, 32, msgs ? msgs + offs[i] : nullptr, (size_t)(offs[i + 1] - offs[i]), c);
                if (on_host) {
                    const uint8_t why = verify_one(vks + 32 * i, sigs + 64 * i, c);
                    ok_out[i] = why == RJ_OK;
                    if (reason_out) reason_out[i] = why;
                } else {
                    memcpy(&cs[(i - first) * 64], c, 32);
                    memcpy(&cs[(i - first) * 64 + 32], sigs + 64 * i + 32, 32);
                }
            }
        };
        zkrt::run_threads(nth, work);
    };
    if (on_host) {
        hash_range(0, n);
        return ZK_OK;
    }
    ZK_TRY(zkrt::use_device(device));
    zkrt::DevBuf in, out;
    in.is_public = out.is_public = true;
    constexpr size_t SLICE = (size_t)1 << 19;   // signatures per launch pair
    const std::vector<uint32_t>& gtab = gtable();
    std::vector<uint8_t> stage;
    std::vector<uint32_t> back;
    for (size_t first = 0; first < n; first += SLICE) {
        const size_t np = std::min(SLICE, n - first), head = GTAB_WORDS * 4 + np * 64;
        // in: gtab | vk_i, Rbar_i | c_i, S_i.   out: x, y of the 2 np points | their statuses | the np reasons
        ZK_TRY(in.ensure(head + np * 64));
        ZK_TRY(out.ensure(np * (128 + 8 + 4)));
        stage.resize(head);
        memcpy(stage.data(), gtab.data(), GTAB_WORDS * 4);
        for (size_t i = 0; i < np; i++) {
            memcpy(&stage[GTAB_WORDS * 4 + i * 64], vks + 32 * (first + i), 32);
            memcpy(&stage[GTAB_WORDS * 4 + i * 64 + 32], sigs + 64 * (first + i), 32);
        }
        HIP_TRY(hipMemcpyAsync(in.p, stage.data(), head, hipMemcpyHostToDevice, zkrt::g_stream));
        const uint32_t* d_gtab = in.as<uint32_t>();
        const uint32_t *d_enc = d_gtab + GTAB_WORDS, *d_cs = d_enc + np * 16;
        uint32_t* d_xy = out.as<uint32_t>();
        uint32_t *d_status = d_xy + np * 32, *d_reason = d_status + np * 2;
        {
            zkrt::ProfScope ps("rj_decode");
            ZK_LAUNCH(k_rj_decode, dim3((unsigned)((2 * np + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_enc, d_xy, d_status, (uint32_t)(2 * np));
        }
        HIP_TRY(hipGetLastError());
        cs.resize(np * 64);
        hash_range(first, np);   // beside the decode kernel
        HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(d_cs), cs.data(), np * 64, hipMemcpyHostToDevice, zkrt::g_stream));
        {
            zkrt::ProfScope ps("rj_check");
            ZK_LAUNCH(k_rj_check, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_gtab, (const uint32_t*)d_xy,
                      (const uint32_t*)d_status, d_cs, d_reason, (uint32_t)np);
        }
        HIP_TRY(hipGetLastError());
        back.resize(np);
        HIP_TRY(hipMemcpyAsync(back.data(), d_reason, np * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        for (size_t i = 0; i < np; i++) {
            ok_out[first + i] = back[i] == RJ_OK;
            if (reason_out) reason_out[first + i] = (uint8_t)back[i];
        }
    }
    return ZK_OK;
}

}  // namespace zkrj
