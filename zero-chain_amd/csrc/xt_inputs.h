// IntoXY for a batch of Jubjub encodings: the public inputs of a transfer extrinsic from its bytes.
//
// PublicInputBuilder::push (modules/zk-system/src/input_builder.rs:15-27) calls IntoXY on every point of an extrinsic
// (core/primitives/src/{enc_key,left_ciphertext,right_ciphertext,nonce,g_epoch,sig_vk}.rs): edwards::Point::read
// (core/jubjub/src/curve/edwards.rs:92-165: y with the sign of x in the top bit, x by a square root in Fr), as_prime_order
// (:319-330: [s]P == O for the order s of the prime-order subgroup) and the affine pair (x, y) - two consecutive public
// inputs of verify_proof.  Eleven points per confidential transfer, fifty-two per anonymous one.
//
// Two forms, the same bytes:
//   host    zkwit::decode_point + zkwit::is_prime_order (transfer_witness.h) on the zk_set_host_threads pool
//   device  k_into_xy, one lane per point.  A point is one serial chain of Fr products and the chain is the whole cost
//           (11 264 lanes of a 1024-transfer block are a sixth of the machine at one wave per SIMD), so the kernel is built to
//           keep it short (2.55 ms for the 11 264 points of 1024 transfers, against 61 ms on 16 host threads) - about 3 200
//           dependent products per point where the witness kernels' decode_point / is_prime_order
//           pair (witness_gpu.h) takes about 4 500:
//             1 / (d y^2 + 1)   one exponentiation by r - 2 in fixed 4-bit windows                    ~330
//             square root       ONE exponentiation w = a^((q - 1) / 2), r - 1 = 2^32 q, in 4-bit windows; x = a w, b = x w
//                               = a^q; Tonelli-Shanks on b; existence decided by x^2 == a at the end   ~290 + <= 500
//             [s]P              s recoded at compile time into signed digits +-1, +-3, +-5, +-7 (width-4 NAF: 252
//                               doublings, 51 additions); doubling dbl-2008-hwcd for a = -1 (4M + 4S, 3M + 4S where T is
//                               not read); additions against P, 3P, 5P, 7P cached as (Y + X, Y - X, 2 d T, 2 Z): 7M  ~2 200
//           The two window tables (a^1 .. a^15; the four cached multiples) live in LDS, [slot][word][lane]: 32 KB per
//           64-lane block, every lane in its own bank, nothing in scratch memory.
// The inputs are public: nothing here is constant-time, and the buffers are freed without the wipe.
#pragma once
#include "dev_field.h"
#include "host_common.h"
#include "host_math.h"
#include "transfer_witness.h"

namespace zkxt {

using zkdev::Fr;
using zkrt::fail;

enum { INTO_XY_OK = 0, INTO_XY_NOT_IN_FIELD = 1, INTO_XY_NOT_ON_CURVE = 2, INTO_XY_NOT_PRIME_ORDER = 3 };
// ZKAMD_INTO_XY_HOST_MAX: points up to which the host form runs.  Measured crossover (profiles/r10_xt_verify_probe.json, 16 host
// threads): the kernel is 2.55-2.65 ms whatever the batch holds, the host form 1.84 ms at 256 points and 4.22 ms at 704.
constexpr size_t INTO_XY_HOST_MAX = 384;

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
// [s](x, y) == O ?
ZK_DI bool is_prime_order(const Lds& L, const Fr& x, const Fr& y, const Fr& d2) {
    constexpr NafDigits S = digits_order();
    const EP p1{x, y, Fr::one(), mul(x, y)};
    cache_put(L, 0, p1, d2);
    cache_put(L, 3, ext_dbl(p1, true), d2);   // 2P, in the place of 7P until 7P is written
    EP q = p1;
#pragma unroll 1
    for (uint32_t i = 1; i < 4; i++) {   // 3P, 5P, 7P = P, 3P, 5P + 2P
        q = ext_add_cached(L, q, 3, false, true);
        cache_put(L, i, q, d2);
    }
    EP acc{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
#pragma unroll 1
    for (int i = S.top; i >= 0; i--) {
        const int v = S.d[i];
        acc = ext_dbl(acc, v != 0);
        if (v) acc = ext_add_cached(L, acc, (uint32_t)((v < 0 ? -v : v) >> 1), v < 0, false);
    }
    return acc.X.is_zero() && acc.Y == acc.Z;
}

// enc: n x 8 words.  xy: n x 16 words, x then y, plain little-endian canonical; zero where refused.  status: n words.
static __global__ void __launch_bounds__(64)
k_into_xy(const uint32_t* enc, uint32_t* xy, uint32_t* status, uint32_t n) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Lds L{table + threadIdx.x};
    Fr y;
    {
        const uint4* q = reinterpret_cast<const uint4*>(enc + (size_t)t * 8);
        const uint4 lo = q[0], hi = q[1];
        y.l[0] = lo.x; y.l[1] = lo.y; y.l[2] = lo.z; y.l[3] = lo.w;
        y.l[4] = hi.x; y.l[5] = hi.y; y.l[6] = hi.z; y.l[7] = hi.w;
    }
    const bool sign = (y.l[7] >> 31) != 0;
    y.l[7] &= 0x7fffffffu;
    uint32_t st = INTO_XY_OK;
    Fr x = Fr::zero();
    {
        uint32_t bo = 0, co;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            (void)__builtin_subc(y.l[i], zkdev::FrCfg::P[i], bo, &co);
            bo = co;
        }
        if (bo == 0) st = INTO_XY_NOT_IN_FIELD;
    }
    if (st == INTO_XY_OK) {
        Fr d;
        {
            const uint64_t dp[4] = ZK_JUBJUB_D_PLAIN_64;
#pragma unroll
            for (int i = 0; i < 8; i++) d.l[i] = (uint32_t)(dp[i >> 1] >> (32 * (i & 1)));
        }
        d = zkdev::to_mont(d);
        const Fr ym = zkdev::to_mont(y);
        const Fr y2 = sqr(ym);
        constexpr PowDigits EI = digits_inverse();
        const Fr den_inv = pow_windows(L, add(mul(d, y2), Fr::one()), EI);   // d y^2 + 1 = 0 has no solution
        const Fr x2 = mul(sub(y2, Fr::one()), den_inv);
        Fr xm;
        if (!sqrt_one_pow(L, x2, &xm)) {
            st = INTO_XY_NOT_ON_CURVE;
        } else {
            x = zkdev::from_mont(xm);
            if (((x.l[0] & 1u) != 0) != sign) {
                xm = neg(xm);
                x = neg(x);
            }
            if (!is_prime_order(L, xm, ym, dbl(d))) st = INTO_XY_NOT_PRIME_ORDER;
        }
    }
    if (st != INTO_XY_OK) x = y = Fr::zero();
    uint4* o = reinterpret_cast<uint4*>(xy + (size_t)t * 16);
    o[0] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
    o[1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    o[2] = make_uint4(y.l[0], y.l[1], y.l[2], y.l[3]);
    o[3] = make_uint4(y.l[4], y.l[5], y.l[6], y.l[7]);
    status[t] = st;
}

// ---- host form: decode_prime_order's arithmetic, one point
inline uint8_t into_xy_one(const uint8_t b[32], uint8_t xy[64]) {
    memset(xy, 0, 64);
    uint64_t v[4];
    zkrt::load_scalar_le(b, v);
    v[3] &= 0x7fffffffffffffffull;
    if (zkhost::Fr::geq_p(v)) return INTO_XY_NOT_IN_FIELD;
    zkwit::JPoint p;
    if (!zkwit::decode_point(b, &p)) return INTO_XY_NOT_ON_CURVE;
    if (!zkwit::is_prime_order(p)) return INTO_XY_NOT_PRIME_ORDER;
    const zkhost::Fr x = p.x.from_mont(), y = p.y.from_mont();
    memcpy(xy, x.l, 32);
    memcpy(xy + 32, y.l, 32);
    return INTO_XY_OK;
}

// the workspaces of the device form (public data: no wipe)
struct IntoXyBufs {
    zkrt::DevBuf in, out;
    IntoXyBufs() { in.is_public = out.is_public = true; }
};

// IntoXY for n encodings (zk_jubjub_into_xy).  device < 0, or n <= ZKAMD_INTO_XY_HOST_MAX (read per call; 0 = always the
// device form): the host form.  Else the kernel on the library stream of `device`, coordinates and statuses back in one copy.
inline zk_status into_xy(const uint8_t* points, size_t n, int device, IntoXyBufs* bufs, uint8_t* xy_out, uint8_t* status_out) {
    if (!n) return ZK_OK;
    const char* e = getenv("ZKAMD_INTO_XY_HOST_MAX");
    const size_t host_max = e && *e ? (size_t)strtoull(e, nullptr, 10) : INTO_XY_HOST_MAX;
    if (device < 0 || n <= host_max) {
        const unsigned nth = zkrt::host_threads(n, 64);
        auto work = [&](unsigned t) {
            for (size_t i = n * t / nth; i < n * (t + 1) / nth; i++) status_out[i] = into_xy_one(points + i * 32, xy_out + i * 64);
        };
        zkrt::run_threads(nth, work);
        return ZK_OK;
    }
    ZK_TRY(zkrt::use_device(device));
    IntoXyBufs local;
    if (!bufs) bufs = &local;
    constexpr size_t SLICE = (size_t)1 << 20;   // points per launch
    std::vector<uint32_t> back;
    for (size_t first = 0; first < n; first += SLICE) {
        const size_t np = std::min(SLICE, n - first);
        ZK_TRY(bufs->in.ensure(np * 32));
        ZK_TRY(bufs->out.ensure(np * 68));
        HIP_TRY(hipMemcpyAsync(bufs->in.p, points + first * 32, np * 32, hipMemcpyHostToDevice, zkrt::g_stream));
        uint32_t* d_xy = bufs->out.as<uint32_t>();
        {
            zkrt::ProfScope ps("into_xy");
            ZK_LAUNCH(k_into_xy, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, zkrt::g_stream, (const uint32_t*)bufs->in.as<uint32_t>(), d_xy,
                      d_xy + np * 16, (uint32_t)np);
        }
        HIP_TRY(hipGetLastError());
        back.resize(np * 17);
        HIP_TRY(hipMemcpyAsync(back.data(), bufs->out.p, np * 68, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(xy_out + first * 64, back.data(), np * 64);
        for (size_t i = 0; i < np; i++) status_out[first + i] = (uint8_t)back[np * 16 + i];
    }
    return ZK_OK;
}

}  // namespace zkxt
