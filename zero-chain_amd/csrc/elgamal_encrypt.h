// ElGamal encryption of a batch under many keys (zk_elgamal_encrypt_dev): Ciphertext::encrypt and neg_encrypt
// (core/proofs/src/no_std_aliases/elgamal.rs:46-63, crypto_components.rs:181-187) and MultiCiphertexts::encrypt
// (crypto_components.rs:60-125, 168-217) as a stage with a device form.  Included by wallet.cpp below anon_derive.h (its Encodings
// and ld_ep; hd_keys.h's fixed_mul and table; wallet_stage.h's point_lane and BoothMul), and by no other unit.
//
// Group i has ONE randomness r_i and k keys: right_i = [r_i]G, left_ij = [v_ij]G + [r_i]pk_ij, G the generator of
// zk_elgamal_encrypt.  A key that Point::read or as_prime_order refuses is a status of its own left and of nothing else.
//   both    the argument checks (k, the values, the randomness), in one order and with one wording, before anything is written
//   host    (zk_set_host_threads pool) the arithmetic of zk_elgamal_encrypt: every DISTINCT key of the call decoded once
//           (read_prime_order); then the lefts shared out key by key - jubjub_var_mul and, where v != 0, jubjub_fixed_mul_ext of |v|
//           with x negated for v < 0 - with [r]G of a group beside its first key, and one batch_to_affine per thread
//   device  two launches per slice of groups on the library stream, one wave per block, nothing in scratch memory:
//     k_enc_points     lane kinds split at wave boundaries (every count but the last is padded to 64: a wave takes one path)
//         decode       one per DISTINCT key encoding of the slice: wallet_stage.h point_lane's first kind - read_point +
//                      is_prime_order, a zkxt::INTO_XY_* status (~2 800 dependent products).  A payout to one key repeated, or a
//                      ring shared by neighbours, is decoded once.
//         variable     one per (group, key): point_lane's second kind with BoothMul - [r_i] pk over signed fixed windows of 3 bits,
//                      all lanes adding at the same 85 positions (~3 350 with read_point).  The k lanes of a group read ONE copy
//                      of r_i (GroupMul: BoothMul's scalar indexed by group).
//         randomness   one per group: [r_i]G by hd_keys.h fixed_mul over the resident positional table (device_table), 43 windows
//                      of 6 bits (~300)
//         value        one per (group, key) with v != 0: [|v|]G by the same fixed_mul over the low VALUE_WINDOWS = 6 windows alone
//                      (|v| < 2^32: bits 0 .. 31, and the signed digit of window 5 is at most 4, so it carries nothing on) (~45).
//                      The sign is not applied here.
//                      All but the decode lanes leave X Y Z T.  LDS is k_keys_points': 17 slots x 32 x 64 = 34 816 B.
//     k_enc_combine    one lane per output point, n k lefts then n rights: the source, for a left with v != 0 plus the value lane's
//                      point with x (and T) negated where v < 0, one inversion (pow_windows, ~330), Point::write's bytes and the
//                      status; a refused left is 32 zero bytes.  LDS: pow_windows' 16 slots, 32 768 B.
//   Built for gfx950 both kernels report no scratch memory (DESIGN.md 4.6.1 has the resource lines).
// Both forms write the same bytes and the same statuses, and refuse the same arguments with the same message.
// Secrets: the randomness is the sender's.  On the device it and everything derived from it ([r]pk, [r]G, the values' points) live
// in DevBufs of the call, zeroed before they are released (zk_memory_stats counts them), on success and on every failure; host
// copies are wiped on every way out.  The device form is NOT constant-time: a zero digit of a lane's scalar skips that lane's
// addition, and a value of zero has no lane; the host form multiplies with jubjub_var_mul / jubjub_fixed_mul_ext, whose steps do
// not depend on the scalar.
#pragma once
#include "anon_derive.h"

namespace zkenc {

using zkdev::Fr;
using zkrt::fail;
using zkxt::EP;
using zkxt::Lds;

// ZKAMD_ENCRYPT_HOST_MAX: left ciphertexts (n k) up to which the host form runs (read per call; 0 = always the kernels).  Measured
// (profiles/r33_encrypt_probe.json, 16 host threads, every key distinct): the device form is 3.0 - 3.3 ms from 1 to 1024 lefts; the
// host form is 1.56 ms at 64 lefts (k = 1), 2.98 at 192 (16 groups of 12) against 3.07, 3.12 at 192 (64 groups of 3) against 3.06 and
// 3.93 at 256 against 3.04 - 192 is the largest probed n k at which the host form is still the faster one.
constexpr size_t HOST_MAX = 192;
constexpr size_t K_MAX = 16;
constexpr size_t SLICE = 4096;   // groups per pair of launches
constexpr uint32_t VALUE_WINDOWS = 6, NONE = 0xffffffffu;
constexpr int64_t VALUE_BOUND = (int64_t)1 << 32;
static_assert(VALUE_WINDOWS * zkhd::WINDOW >= 32 + 1 && VALUE_WINDOWS <= (uint32_t)zkhd::WINDOWS, "the windows of a 32-bit value and the carry of its top digit");
static_assert(zkhd::SLOT_SCALAR == zkscan::KEYS_SLOT_SCALAR && zkhd::LDS_WORDS * 4 == zkscan::KEYS_LDS_BYTES, "one LDS layout for every lane kind");

inline size_t host_max() {
    const char* e = getenv("ZKAMD_ENCRYPT_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
}

// ---- device
// BoothMul with the scalar of lane r's GROUP: lane r is key r % k of group r / k
struct GroupMul {
    const uint32_t* scalars;
    uint32_t k;
    ZK_DI EP operator()(const Lds& L, uint32_t r, const Fr& xm, const Fr& ym, const Fr& d2) const {
        return zkscan::BoothMul{scalars}(L, r / k, xm, ym, d2);
    }
};
// enc: d64 x 8 words (n_dec used).  venc: n_var x 8 words, the key of every (group, key).  gsc: n_grp x 8 plain words, the
// randomness of every group.  k: keys per group.  tab: zkhd::TAB_WORDS.  vals: n_val words, |v| of every value lane.
// xy: n_dec x 16 words, status: n_dec words (point_lane's).  proj: (n_var + n_grp + n_val) x 32 words, X Y Z T.
static __global__ void __launch_bounds__(64)
k_enc_points(const uint32_t* enc, uint32_t n_dec, uint32_t d64, const uint32_t* venc, const uint32_t* gsc, uint32_t k, uint32_t n_var, uint32_t v64,
             const uint32_t* tab, uint32_t n_grp, uint32_t g64, const uint32_t* vals, uint32_t n_val, uint32_t* xy, uint32_t* status, uint32_t* proj) {
    ZK_SHARED uint32_t table[zkscan::KEYS_LDS_SLOTS * 8 * 64];
    const Lds L{table + threadIdx.x};
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t < d64 + v64) {
        zkscan::point_lane(L, enc, n_dec, d64, venc, n_var, GroupMul{gsc, k}, xy, status, proj);
        return;
    }
    const uint32_t f = t - d64 - v64;
    uint32_t at, windows = (uint32_t)zkhd::WINDOWS;
    if (f < g64) {
        if (f >= n_grp) return;
        L.st(zkhd::SLOT_SCALAR, zkrj::ld_fr(gsc + (size_t)f * 8));
        at = n_var + f;
    } else {
        const uint32_t m = f - g64;
        if (m >= n_val) return;
        Fr v = Fr::zero();
        v.l[0] = vals[m];
        L.st(zkhd::SLOT_SCALAR, v);
        windows = VALUE_WINDOWS;
        at = n_var + n_grp + m;
    }
    const EP p = zkhd::fixed_mul<false>(L, tab, nullptr, windows);
    uint32_t* o = proj + (size_t)at * 32;
    zkscan::st_fr(o, p.X);
    zkscan::st_fr(o + 8, p.Y);
    zkscan::st_fr(o + 16, p.Z);
    zkscan::st_fr(o + 24, p.T);
}
// src: n x 4 words - the lane's source in proj, its addend there (or NONE), whether the addend is negated, the decode lane of its
// key (or NONE: a right).  dstatus: k_enc_points' status.  out: n x 8 words, Point::write (zero where the key is refused);
// status: n words.  (Z is never zero where the key is accepted: the addition law is complete on prime-order points.)
static __global__ void __launch_bounds__(64)
k_enc_combine(const uint32_t* proj, const uint32_t* dstatus, const uint32_t* src, uint32_t n, uint32_t* out, uint32_t* status) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Lds L{table + threadIdx.x};
    const uint4 s = reinterpret_cast<const uint4*>(src)[t];
    const uint32_t st = s.w == NONE ? (uint32_t)zkxt::INTO_XY_OK : dstatus[s.w];
    status[t] = st;
    uint32_t* o = out + (size_t)t * 8;
    if (st != zkxt::INTO_XY_OK) {
        zkscan::st_fr(o, Fr::zero());
        return;
    }
    EP p = zkanon::ld_ep(proj + (size_t)s.x * 32);
    if (s.y != NONE) {
        EP q = zkanon::ld_ep(proj + (size_t)s.y * 32);
        if (s.z) {
            q.X = neg(q.X);
            q.T = neg(q.T);
        }
        p = zkxt::ext_add(p, q, zkxt::jubjub_d2());
    }
    constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
    const Fr zi = zkxt::pow_windows(L, p.Z, EI);
    zkscan::st_fr(o, zkxt::point_words(mul(p.X, zi), mul(p.Y, zi)));
}

// ---- host side
// what both forms refuse, before either writes anything
inline zk_status check_arguments(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys, const uint8_t* left_out,
                                 const uint8_t* right_out, const uint8_t* status_out) {
    if (k < 1 || k > K_MAX) return fail(ZK_ERR_INVALID_ARGUMENT, "k must be 1 .. " + std::to_string(K_MAX));
    if (!values || !randomness || !enc_keys || !left_out || !right_out || !status_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (~(size_t)0 >> 6) / k) return fail(ZK_ERR_INVALID_ARGUMENT, "n k is too large");
    for (size_t t = 0; t < n * k; t++)
        if (values[t] <= -VALUE_BOUND || values[t] >= VALUE_BOUND) return fail(ZK_ERR_INVALID_ARGUMENT, "value " + std::to_string(t) + " is outside (-2^32, 2^32)");
    for (size_t i = 0; i < n; i++) {
        uint64_t r[4];
        WipeOnExit wipe_r{r, sizeof(r)};
        zkrt::load_scalar_le(randomness + 32 * i, r);
        if (!fs_lt_mod(r)) return fail(ZK_ERR_INVALID_ARGUMENT, "randomness " + std::to_string(i) + " is not a canonical Fs scalar");
    }
    return ZK_OK;
}
inline uint32_t magnitude(int64_t v) { return (uint32_t)(v < 0 ? -v : v); }

inline zk_status encrypt_host(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys, uint8_t* left_out,
                              uint8_t* right_out, uint8_t* status_out) {
    (void)zkwit::tables();
    // the distinct keys of the call, each decoded once
    zkanon::Encodings E(n * k);
    std::vector<uint32_t> ids(n * k);
    for (size_t t = 0; t < n * k; t++) ids[t] = E.put(enc_keys + 32 * t);
    std::vector<zkwit::JPoint> keys(E.size());
    std::vector<uint8_t> refusal(E.size());
    ZK_TRY(zkrt::for_each_status(E.size(), 64, [&](size_t d) -> zk_status {
        refusal[d] = zkscan::read_prime_order(&E.enc[32 * d], &keys[d]);
        return ZK_OK;
    }));
    // the lefts over the threads, key by key (one group of 12 is twelve items, not one); [r]G of a group with its first key
    return zkrt::for_each_range(n * k, 64, [&](size_t t0, size_t t1) -> zk_status {
        std::vector<zkwit::EPoint> proj;
        proj.reserve(t1 - t0 + (t1 - t0) / k + 2);   // (never moves: what is wiped below is all of it)
        uint64_t r[4];
        WipeOnExit wipe_p{proj.data(), proj.capacity() * sizeof(zkwit::EPoint)}, wipe_r{r, sizeof(r)};
        for (size_t t = t0; t < t1; t++) {
            zkrt::load_scalar_le(randomness + 32 * (t / k), r);
            // left = v G + r pk, right = r G  (no_std_aliases/elgamal.rs:46-63; neg_encrypt: crypto_components.rs:181-187)
            if ((status_out[t] = refusal[ids[t]]) != 0) {
                proj.push_back(zkwit::ext_zero());
            } else {
                proj.push_back(jubjub_var_mul(keys[ids[t]], r));
                if (values[t] != 0) {
                    const uint64_t mag[4] = {magnitude(values[t]), 0, 0, 0};
                    zkwit::EPoint vg = jubjub_fixed_mul_ext(mag);
                    if (values[t] < 0) vg = zkwit::EPoint{zkhost::Fr::zero() - vg.X, vg.Y, vg.Z, zkhost::Fr::zero() - vg.T};
                    proj.back() = zkwit::ext_add(vg, proj.back());
                }
            }
            if (t % k == 0) proj.push_back(jubjub_fixed_mul_ext(r));
        }
        std::vector<zkwit::JPoint> aff(proj.size());
        WipeOnExit wipe_a{aff.data(), aff.size() * sizeof(zkwit::JPoint)};
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        const zkwit::JPoint* a = aff.data();
        for (size_t t = t0; t < t1; t++, a++) {
            if (status_out[t]) {
                memset(left_out + 32 * t, 0, 32);
            } else {
                jubjub_encode(a->x, a->y, left_out + 32 * t);
            }
            if (t % k == 0) {
                a++;
                jubjub_encode(a->x, a->y, right_out + 32 * (t / k));
            }
        }
        return ZK_OK;
    });
}

inline zk_status encrypt_device(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys, int device, uint8_t* left_out,
                                uint8_t* right_out, uint8_t* status_out) {
    ZK_TRY(zkrt::use_device(device));
    const uint32_t* tab = nullptr;
    ZK_TRY(zkhd::device_table(device, &tab));
    size_t slice = SLICE;
    if (const char* e = zkrt::hook_env("ZKAMD_DEBUG_ENCRYPT_SLICE")) slice = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));   // test hook: several slices of a few groups
    zkrt::DevBuf in, out;   // the randomness and its multiples: zeroed before they go back, on every way out of this function
    std::vector<uint32_t> hin, back, ids;   // hin: the slice as it is uploaded, the randomness among it; back: bytes and statuses - public
    struct WipeWords {
        std::vector<uint32_t>& v;
        ~WipeWords() {
            if (!v.empty()) explicit_bzero(v.data(), v.size() * 4);
        }
    } wipe_hin{hin};
    auto pad = [](size_t v, size_t to) { return (v + to - 1) / to * to; };
    for (size_t first = 0; first < n; first += slice) {
        const size_t np = std::min(slice, n - first), nv = np * k, nc = nv + np;
        const int64_t* val = values + first * k;
        // the distinct keys of the slice, and the lane of each
        zkanon::Encodings E(nv);
        ids.resize(nv);
        size_t nval = 0;
        for (size_t t = 0; t < nv; t++) {
            ids[t] = E.put(enc_keys + 32 * (first * k + t));
            nval += val[t] != 0;
        }
        const size_t nd = E.size(), d64 = pad(nd, 64), v64 = pad(nv, 64), g64 = pad(np, 64);
        // in: encodings | keys | randomness | values (padded to 4) | combine sources
        const size_t w_venc = d64 * 8, w_gsc = w_venc + nv * 8, w_val = w_gsc + np * 8, w_src = w_val + pad(nval, 4), in_words = w_src + nc * 4;
        // out: bytes | statuses (padded to 4) || the decode lanes' statuses (padded to 4) | their coordinates | the projective points
        const size_t w_st = nc * 8, back_words = w_st + pad(nc, 4), w_dst = back_words, w_xy = w_dst + pad(nd, 4), w_proj = w_xy + nd * 16,
                     out_words = w_proj + (nv + np + nval) * 32;
        if (!hin.empty()) explicit_bzero(hin.data(), hin.size() * 4);   // (before assign() may move it)
        hin.assign(in_words, 0);
        back.resize(std::max(back.size(), back_words));
        memcpy(hin.data(), E.enc.data(), nd * 32);
        memcpy(&hin[w_venc], enc_keys + 32 * first * k, nv * 32);
        memcpy(&hin[w_gsc], randomness + 32 * first, np * 32);
        uint32_t* src = &hin[w_src];
        for (size_t t = 0, m = 0; t < nc; t++) {   // the lefts, then the rights: [r]G of group t - nv
            src[4 * t] = (uint32_t)t;
            src[4 * t + 1] = src[4 * t + 3] = NONE;
            if (t >= nv) continue;
            src[4 * t + 3] = ids[t];
            if (val[t] == 0) continue;
            hin[w_val + m] = magnitude(val[t]);
            src[4 * t + 1] = (uint32_t)(nv + np + m++);
            src[4 * t + 2] = val[t] < 0 ? 1u : 0u;
        }
        ZK_TRY(in.ensure(in_words * 4));
        ZK_TRY(out.ensure(out_words * 4));
        const uint32_t* d_in = in.as<const uint32_t>();
        uint32_t* d_out = out.as<uint32_t>();
        {
            zkrt::ProfScope ps("encrypt_upload");
            HIP_TRY(hipMemcpyAsync(in.p, hin.data(), in_words * 4, hipMemcpyHostToDevice, zkrt::g_stream));
        }
        {
            zkrt::ProfScope ps("encrypt_points");
            ZK_LAUNCH(k_enc_points, dim3((unsigned)((d64 + v64 + g64 + pad(nval, 64)) / 64)), dim3(64), 0, zkrt::g_stream, d_in, (uint32_t)nd, (uint32_t)d64,
                      d_in + w_venc, d_in + w_gsc, (uint32_t)k, (uint32_t)nv, (uint32_t)v64, tab, (uint32_t)np, (uint32_t)g64, d_in + w_val, (uint32_t)nval,
                      d_out + w_xy, d_out + w_dst, d_out + w_proj);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps("encrypt_combine");
            ZK_LAUNCH(k_enc_combine, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_out + w_proj, d_out + w_dst, d_in + w_src, (uint32_t)nc,
                      d_out, d_out + w_st);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps("encrypt_download");
            HIP_TRY(hipMemcpyAsync(back.data(), out.p, back_words * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        }
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(left_out + 32 * first * k, back.data(), nv * 32);
        memcpy(right_out + 32 * first, back.data() + nv * 8, np * 32);
        for (size_t t = 0; t < nv; t++) status_out[first * k + t] = (uint8_t)back[w_st + t];
    }
    return ZK_OK;
}

// the stage: the form by ZKAMD_ENCRYPT_HOST_MAX
inline zk_status encrypt(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys, int device, uint8_t* left_out,
                         uint8_t* right_out, uint8_t* status_out) {
    if (n == 0) return ZK_OK;
    ZK_TRY(check_arguments(n, k, values, randomness, enc_keys, left_out, right_out, status_out));
    return device < 0 || n * k <= host_max() ? encrypt_host(n, k, values, randomness, enc_keys, left_out, right_out, status_out)
                                             : encrypt_device(n, k, values, randomness, enc_keys, device, left_out, right_out, status_out);
}

}  // namespace zkenc
