// ElGamal encryption of a batch under many keys (zk_elgamal_encrypt_dev): Ciphertext::encrypt and neg_encrypt
// (core/proofs/src/no_std_aliases/elgamal.rs:46-63, crypto_components.rs:181-187) and MultiCiphertexts::encrypt
// (crypto_components.rs:60-125, 168-217) as a stage with a device form.  Included by wallet.cpp below anon_derive.h (for
// derive_stage.h, the stage they share), and by no other unit.
//
// Group i has ONE randomness r_i and k keys: right_i = [r_i]G, left_ij = [v_ij]G + [r_i]pk_ij, G the generator of
// zk_elgamal_encrypt.  A key that Point::read or as_prime_order refuses is a status of its own left and of nothing else.
//   both    the argument checks (k, the values, the randomness), in one order and with one wording, before anything is written
//   host    (zk_set_host_threads pool) the arithmetic of zk_elgamal_encrypt: every DISTINCT key of the call decoded once
//           (read_prime_order); then the lefts shared out key by key - jubjub_var_mul and, where v != 0, jubjub_fixed_mul_ext of |v|
//           with x negated for v < 0 - with [r]G of a group beside its first key, and one batch_to_affine per thread
//   device  derive_stage.h's two launches per slice of groups, the lanes described as data.  The pool is the randomness of every
//           group, then |v| of every v != 0:
//         decode       one per DISTINCT key encoding of the slice: a payout to one key repeated, or a ring shared by neighbours, is
//                      decoded once
//         variable     one per (group, key): [r_i] pk, the k lanes of a group reading ONE copy of r_i
//         fixed        one per group, 43 windows: [r_i]G; padding to 64; then one per (group, key) with v != 0 over the low
//                      VALUE_WINDOWS = 6 windows alone: [|v|]G (|v| < 2^32: bits 0 .. 31, and the signed digit of window 5 is at most
//                      4, so it carries nothing on) (~45 products).  The sign is not applied here.
//         combine      8 words each, n k lefts then n rights: the source, for a left with v != 0 plus the value lane's point, negated
//                      where v < 0; a left answers for its key's decode lane: the status, and 32 zero bytes where it is refused
// Both forms write the same bytes and the same statuses, and refuse the same arguments with the same message.
// Secrets: the randomness is the sender's.  On the device it and everything derived from it ([r]pk, [r]G, the values' points) live
// in the DevBufs of the call's Stage, zeroed before they are released (zk_memory_stats counts them), on success and on every failure; host
// copies are wiped on every way out.  The device form is NOT constant-time: a zero digit of a lane's scalar skips that lane's
// addition, and a value of zero has no lane; the host form multiplies with jubjub_var_mul / jubjub_fixed_mul_ext, whose steps do
// not depend on the scalar.
#pragma once
#include "anon_derive.h"

namespace zkenc {

using zkrt::fail;
using zkstage::NONE;

// ZKAMD_ENCRYPT_HOST_MAX: left ciphertexts (n k) up to which the host form runs (read per call; 0 = always the kernels).  Measured
// (profiles/r33_encrypt_probe.json, 16 host threads, every key distinct): the device form is 3.0 - 3.3 ms from 1 to 1024 lefts; the
// host form is 1.56 ms at 64 lefts (k = 1), 2.98 at 192 (16 groups of 12) against 3.07, 3.12 at 192 (64 groups of 3) against 3.06 and
// 3.93 at 256 against 3.04 - 192 is the largest probed n k at which the host form is still the faster one.
constexpr size_t HOST_MAX = 192;
constexpr size_t K_MAX = 16;
constexpr size_t SLICE = 4096;   // groups per pair of launches
constexpr uint32_t VALUE_WINDOWS = 6;
constexpr int64_t VALUE_BOUND = (int64_t)1 << 32;
static_assert(VALUE_WINDOWS * zkhd::WINDOW >= 32 + 1 && VALUE_WINDOWS <= (uint32_t)zkhd::WINDOWS, "the windows of a 32-bit value and the carry of its top digit");

inline size_t host_max() {
    const char* e = getenv("ZKAMD_ENCRYPT_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
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
    zkstage::Encodings E(n * k);
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
    zkstage::Stage S;   // the randomness and its multiples, on the device and in the upload's host copy: gone on every way out of this function
    std::vector<uint32_t> ids;
    for (size_t first = 0; first < n; first += slice) {
        const size_t np = std::min(slice, n - first), nv = np * k, g64 = zkstage::Stage::pad(np, 64);
        const int64_t* val = values + first * k;
        // the distinct keys of the slice, and the lane of each
        zkstage::Encodings E(nv);
        ids.resize(nv);
        size_t nval = 0;
        for (size_t t = 0; t < nv; t++) {
            ids[t] = E.put(enc_keys + 32 * (first * k + t));
            nval += val[t] != 0;
        }
        S.begin({E.size(), nv, np + nval, g64 + nval, 0, nv + np, 8, true, "encrypt_upload", "encrypt_points", "encrypt_combine", "encrypt_download"});
        memcpy(S.enc, E.enc.data(), E.size() * 32);
        memcpy(S.venc, enc_keys + 32 * first * k, nv * 32);
        memcpy(S.pool, randomness + 32 * first, np * 32);
        auto put = [](uint32_t* at, uint32_t x, uint32_t y, uint32_t z, uint32_t w) { at[0] = x, at[1] = y, at[2] = z, at[3] = w; };
        for (size_t g = 0, t = 0, m = 0; g < np; g++) {
            put(S.fix + 4 * g, (uint32_t)g, (uint32_t)zkhd::WINDOWS, NONE, (uint32_t)(nv + g));   // [r_g]G, which is also the right: combine lane nv + g
            put(S.src + 4 * (nv + g), (uint32_t)(nv + g), NONE, 0, NONE);
            for (size_t j = 0; j < k; j++, t++) {   // the lefts of the group; value lane m behind the groups' wave-padded lanes
                S.vidx[t] = (uint32_t)g;
                const uint32_t value_at = (uint32_t)(nv + np + m);
                put(S.src + 4 * t, (uint32_t)t, val[t] ? value_at : NONE, val[t] < 0, ids[t]);
                if (val[t] == 0) continue;
                S.pool[(np + m) * 8] = magnitude(val[t]);
                put(S.fix + 4 * (g64 + m), (uint32_t)(np + m), VALUE_WINDOWS, NONE, value_at);
                m++;
            }
        }
        ZK_TRY(S.run(tab));
        memcpy(left_out + 32 * first * k, S.out, nv * 32);
        memcpy(right_out + 32 * first, S.out + nv * 8, np * 32);
        for (size_t t = 0; t < nv; t++) status_out[first * k + t] = (uint8_t)S.status[t];
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
