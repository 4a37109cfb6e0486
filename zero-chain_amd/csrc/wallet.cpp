// libzkamd, wallet level: ProofBuilder::gen_proof of the reference for batches of transfers, and the host side of Jubjub it
// is made of.  Replaces, behind the C ABI (include/zkamd.h, "gen_proof"):
//   ProofBuilder::gen_proof          core/proofs/src/confidential.rs:105-172, core/proofs/src/anonymous.rs:97-183
//   key derivation                   core/proofs/src/no_std_aliases/keys.rs:45-198 (SpendingKey::from_seed, ProofGenerationKey,
//                                    DecryptionKey, EncryptionKey), rvk / rsk / nonce
//   elgamal::Ciphertext::encrypt     core/proofs/src/no_std_aliases/elgamal.rs:46-63
//   elgamal::Ciphertext::decrypt     elgamal.rs:85-108 (the host half; the search is witness.cpp's, kernels elgamal_dlog.h)
//   elgamal::Ciphertext::add / sub   elgamal.rs:139-158
//   check_proof + ConfidentialXt / AnonymousXt packing   confidential.rs:208-361, anonymous.rs:200-352
//   redjubjub PrivateKey::sign / PublicKey::verify       core/jubjub/src/redjubjub.rs:73-103, 127-155 (redjubjub.h)
//   a block read with one decryption key                 - (elgamal.rs:85-108 per value, crypto_components.rs:168-220; elgamal_scan.h)
//   BalanceQuery::get_balance_from_decryption_key        zface/src/utils/getter.rs:135-175, for the accounts of a key set (balance_keys.h)
//   ExtendedSpendingKey / ExtendedProofGenerationKey     zface/src/derive/mod.rs:48-228 (master, derive_child, read / write; hd_keys.h)
// Proving itself (witness kernels, row evaluations, the multiexps) is zkamd.cpp's; the only kernels of this unit are the two of
// the signature check (redjubjub.h), the two point kernels of the scans' and the balance query's one point stage (wallet_stage.h),
// its two combines (elgamal_scan.h, balance_keys.h), the two of the key derivation's fixed-base multiplier (hd_keys.h) and the two
// of the derived-point stage (derive_stage.h) behind the anonymous transfer's request -> statement derivation (anon_derive.h) and the
// encryption under many keys (elgamal_encrypt.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <thread>
#include <future>
#include <utility>
#include <chrono>
#include <algorithm>
#include <memory>

#include "../../include/zkamd.h"
#include "gpu_rt.h"
#include <future>
#include "host_common.h"
#include "host_math.h"
#include "blake2s.h"
#include "consts.h"
#include "transfer_witness.h"
#include "handles.h"

using namespace zkrt;
using zkhost::Fr;

// ------------------------------------------------------------------------------------------
// gen_proof: the wallet-level entry of the reference (core/proofs/src/confidential.rs:105-172) for a batch of
// transfers - key derivation (no_std_aliases/keys.rs:132-198), the statement, create_proof, the ElGamal
// ciphertexts (elgamal.rs:46-63), the self-check (check_proof, confidential.rs:208-278) and the packing of
// ConfidentialXt (gen_xt :282-354, the struct :358-370).
// ------------------------------------------------------------------------------------------


namespace {

const uint64_t FS_MOD[4] = ZK_JUBJUB_FS_MODULUS_64;
bool fs_lt_mod(const uint64_t v[4]) {
    for (int i = 3; i >= 0; i--) {
        if (v[i] < FS_MOD[i]) return true;
        if (v[i] > FS_MOD[i]) return false;
    }
    return false;
}
void fs_sub_mod(uint64_t v[4]) {
    zkhost::u128 bo = 0;
    for (int i = 0; i < 4; i++) {
        zkhost::u128 d = (zkhost::u128)v[i] - FS_MOD[i] - bo;
        v[i] = (uint64_t)d;
        bo = (d >> 64) & 1;
    }
}
// (a + b) mod s for a, b < s
void fs_add(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    zkhost::u128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (zkhost::u128)a[i] + b[i];
        out[i] = (uint64_t)c;
        c >>= 64;
    }
    if (!fs_lt_mod(out)) fs_sub_mod(out);   // s < 2^252: the sum never carries out of 256 bits
}
// Fs::to_uniform: a little-endian byte string reduced mod s (bit by bit: off the hot path)
void fs_to_uniform(const uint8_t* le, size_t len, uint64_t out[4]) {
    uint64_t v[4] = {0, 0, 0, 0};
    for (size_t i = len; i-- > 0;)
        for (int b = 7; b >= 0; b--) {
            for (int k = 3; k > 0; k--) v[k] = (v[k] << 1) | (v[k - 1] >> 63);
            v[0] = (v[0] << 1) | ((le[i] >> b) & 1u);
            if (!fs_lt_mod(v)) fs_sub_mod(v);
        }
    memcpy(out, v, 32);
}
// The two scalar multiplications below run on SECRETS (spending / decryption keys, randomness).  Their control flow and their
// table addresses do not depend on the scalar: every step performs the same (complete, unified) Edwards addition with an
// operand picked by masks - entry 0 of a window is the neutral element - and a window's eight entries are all read (VERDICT
// r3 / r4: the digit-dependent `if` of the earlier version).  What remains variable-time is the final conditional
// subtraction inside the host field routines, as in the reference's own Fr (core/pairing/src/bls12_381/fr.rs).
static inline zkhost::Fr ct_pick(uint64_t mask, const zkhost::Fr& a, const zkhost::Fr& b) {   // mask all-ones: a, zero: b
    zkhost::Fr r;
    for (int i = 0; i < 4; i++) r.l[i] = (a.l[i] & mask) | (b.l[i] & ~mask);
    return r;
}
// k * G for the fixed generator, from its 3-bit window tables (k < 2^252)
zkwit::EPoint jubjub_fixed_mul_ext(const uint64_t k[4]) {   // (projective: for callers that bring many to affine form at once)
    const zkwit::Tables& t = zkwit::tables();
    zkwit::EPoint acc = zkwit::ext_zero();
    for (int w = 0; w < 84; w++) {
        const int bit = 3 * w;
        const uint32_t d = (uint32_t)((k[bit >> 6] >> (bit & 63)) | ((bit & 63) > 61 && (bit >> 6) < 3 ? k[(bit >> 6) + 1] << (64 - (bit & 63)) : 0)) & 7u;
        zkwit::JPoint e = t.win[w][0];
        for (uint32_t j = 1; j < 8; j++) {
            const uint64_t m = 0ull - (uint64_t)(j == d);
            e.x = ct_pick(m, t.win[w][j].x, e.x);
            e.y = ct_pick(m, t.win[w][j].y, e.y);
        }
        acc = zkwit::ext_add(acc, zkwit::to_ext(e));
    }
    return acc;
}
zkwit::JPoint jubjub_fixed_mul(const uint64_t k[4]) {
    const zkwit::EPoint acc = jubjub_fixed_mul_ext(k);
    zkwit::JPoint out;
    zkwit::batch_to_affine(&acc, &out, 1);
    return out;
}
// edwards::Point::write (core/jubjub/src/curve/edwards.rs:190-206): y, little-endian, the parity of x in the top bit
void jubjub_encode(const zkhost::Fr& x_mont, const zkhost::Fr& y_mont, uint8_t out[32]) {
    const zkhost::Fr x = x_mont.from_mont(), y = y_mont.from_mont();
    memcpy(out, y.l, 32);
    if (x.l[0] & 1) out[31] |= 0x80;
}

// k * p for a point of the statement (double-and-add over the complete addition law; k < 2^252)
zkwit::EPoint jubjub_var_mul(const zkwit::EPoint& base, const uint64_t k[4]) {
    zkwit::EPoint acc = zkwit::ext_zero();
    const zkwit::EPoint zero = zkwit::ext_zero();
    for (int bit = 251; bit >= 0; bit--) {
        acc = zkwit::ext_add(acc, acc);
        const uint64_t m = 0ull - ((k[bit >> 6] >> (bit & 63)) & 1ull);
        acc = zkwit::ext_add(acc, zkwit::EPoint{ct_pick(m, base.X, zero.X), ct_pick(m, base.Y, zero.Y), ct_pick(m, base.Z, zero.Z),
                                                ct_pick(m, base.T, zero.T)});
    }
    return acc;
}
zkwit::EPoint jubjub_var_mul(const zkwit::JPoint& p, const uint64_t k[4]) { return jubjub_var_mul(zkwit::to_ext(p), k); }

// secrets (spending keys, decryption keys, rsk, the statements that carry them) do not outlive the call that held
// them: wiped on every exit path
struct WipeOnExit {
    void* p;
    size_t n;
    ~WipeOnExit() {
        if (p && n) explicit_bzero(p, n);
    }
};
// request -> statement (+ rsk): ProofGenerationKey::from_spending_key, into_decryption_key, SpendingKey::into_rsk
// Point<E, Unknown>::as_prime_order (core/jubjub/src/curve/edwards.rs:319-330): [s]P == O for the order s of the
// prime-order subgroup.  The reference's typed inputs (EncryptionKey::read keys.rs:269-276, Ciphertext::read
// elgamal.rs:117-133, g_epoch.rs:75) pass through it, so a point with a torsion component is refused by the wallet-level
// entries here too.  The test itself: zkwit::is_prime_order (transfer_witness.h), shared with IntoXY's host form.
zk_status decode_prime_order(const uint8_t b[32], zkwit::JPoint* out, const std::string& what) {
    zkwit::JPoint p;
    if (!zkwit::decode_point(b, &p)) return fail(ZK_ERR_INVALID_ARGUMENT, what + " is not a Jubjub point");
    if (!zkwit::is_prime_order(p)) return fail(ZK_ERR_INVALID_ARGUMENT, what + " is not in the prime-order subgroup");
    if (out) *out = p;
    return ZK_OK;
}

// check_points: decode the four typed inputs and run as_prime_order on them HERE (zk_transfer_derive, a host-only
// entry); gen_proof leaves both to the witness kernels of the chunk (witness_gpu_enqueue typed_inputs: same refusals,
// reported by witness_gpu_finish before the chunk is proved).
zk_status transfer_derive_one(const zk_transfer_request& rq, size_t index, zk_transfer_statement* st, uint8_t rsk[32], bool check_points,
                              bool spread = false) {
    uint64_t sk[4], alpha[4], rnd[4], r[4] = {0, 0, 0, 0};
    WipeOnExit wipe_sk{sk, sizeof(sk)}, wipe_alpha{alpha, sizeof(alpha)}, wipe_rnd{rnd, sizeof(rnd)}, wipe_r{r, sizeof(r)};   // every exit path
    load_scalar_le(rq.spending_key, sk);
    load_scalar_le(rq.alpha, alpha);
    load_scalar_le(rq.randomness, rnd);
    const std::string who = "request " + std::to_string(index) + ": ";
    if (!fs_lt_mod(sk)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "spending_key is not a canonical Fs scalar");
    if (!fs_lt_mod(alpha)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "alpha is not a canonical Fs scalar");
    if (!fs_lt_mod(rnd)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "randomness is not a canonical Fs scalar");
    const zkwit::JPoint pgk = jubjub_fixed_mul(sk);
    memset(st, 0, sizeof(*st));
    st->amount = rq.amount;
    st->remaining_balance = rq.remaining_balance;
    st->fee = rq.fee;
    memcpy(st->randomness, rq.randomness, 32);
    memcpy(st->alpha, rq.alpha, 32);
    jubjub_encode(pgk.x, pgk.y, st->proof_generation_key);
    // keys.rs:166-185: Blake2s("zech_bdk", pgk) with the five top bits dropped
    static const uint8_t person[8] = {'z', 'e', 'c', 'h', '_', 'b', 'd', 'k'};
    zkhash::Blake2s h(person);
    h.update(st->proof_generation_key, 32);
    h.finish(st->dec_key_sender);
    st->dec_key_sender[31] &= 0x07;
    if (check_points) {
        const uint8_t* enc[4] = {rq.enc_key_recipient, rq.enc_balance_left, rq.enc_balance_right, rq.g_epoch};
        static const char* const name[4] = {"enc_key_recipient", "enc_balance_left", "enc_balance_right", "g_epoch"};
        if (spread) {
            // ONE request (the reference's call pattern): the four decodings - a square root and a multiplication by the group
            // order each, 0.09 ms - side by side; the first failure in the order of the fields is the one reported
            std::future<std::pair<zk_status, std::string>> fu[4];
            for (int k = 0; k < 4; k++)
                fu[k] = std::async(std::launch::async, [&, k] {
                    const zk_status rc = decode_prime_order(enc[k], nullptr, who + name[k]);
                    return std::make_pair(rc, rc == ZK_OK ? std::string() : g_err);
                });
            zk_status first = ZK_OK;
            std::string msg;
            for (int k = 0; k < 4; k++) {
                const auto res = fu[k].get();
                if (first == ZK_OK && res.first != ZK_OK) {
                    first = res.first;
                    msg = res.second;
                }
            }
            if (first != ZK_OK) return fail(first, msg);
        } else {
            for (int k = 0; k < 4; k++) ZK_TRY(decode_prime_order(enc[k], nullptr, who + name[k]));
        }
    }
    memcpy(st->enc_key_recipient, rq.enc_key_recipient, 32);
    memcpy(st->enc_balance_left, rq.enc_balance_left, 32);
    memcpy(st->enc_balance_right, rq.enc_balance_right, 32);
    memcpy(st->g_epoch, rq.g_epoch, 32);
    fs_add(sk, alpha, r);   // PrivateKey(sk).randomize(alpha)
    memcpy(rsk, r, 32);
    return ZK_OK;
}
zk_status transfer_derive(const zk_transfer_request* rq, size_t n, zk_transfer_statement* st, uint8_t* rsk, bool check_points) {
    if (n == 0) return ZK_OK;
    (void)zkwit::tables();
    const bool spread = check_points && n * 4 <= host_threads(4 * n, 64);   // a handful of requests: the four decodings of each on their own threads
    return for_each_status(n, 64, [&](size_t i) -> zk_status { return transfer_derive_one(rq[i], i, &st[i], rsk + i * 32, check_points, spread); });
}

}  // namespace

#include "redjubjub.h"   // (here: it signs and hashes with the helpers above)
#include "wallet_stage.h"   // (the point stage of the three below: two point kernels, the device form, the host forms' tail)
#include "elgamal_scan.h"   // (the scan decodes, multiplies and wipes with the helpers above)
#include "scan_keys.h"      // (the same scan for a set of keys: a scalar per hit)
#include "balance_keys.h"   // (the balances of such a set's accounts: the same point kernel, a combine of its own)
#include "hd_keys.h"        // (the children of an extended key and their accounts: a fixed-base multiplier of its own, two kernels)

extern "C" {

zk_status zk_redjubjub_sign(size_t n, const uint8_t* rsk, const uint8_t* t, const uint8_t* msgs, const uint64_t* msg_offsets,
                            uint8_t* sigs_out) try {
    if (n && (!rsk || !t || !msg_offsets || !sigs_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    return zkrj::sign(n, rsk, t, msgs, msg_offsets, sigs_out);
} ZK_ABI_CATCH

zk_status zk_redjubjub_verify_batch(size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                    int device, uint8_t* ok_out, uint8_t* reason_out) try {
    if (n && (!vks || !sigs || !msg_offsets || !ok_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    return zkrj::verify_batch(n, vks, sigs, msgs, msg_offsets, device, ok_out, reason_out);
} ZK_ABI_CATCH

zk_status zk_spending_key_from_seed(const uint8_t* seed, size_t len, uint8_t spending_key_out[32]) try {
    if ((!seed && len) || !spending_key_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    // keys.rs:45-58: Blake2b-512 personalised "zech_ExpandSeed_", then Fs::to_uniform
    static const uint8_t person[16] = {'z', 'e', 'c', 'h', '_', 'E', 'x', 'p', 'a', 'n', 'd', 'S', 'e', 'e', 'd', '_'};
    zkhash::Blake2b h(person);
    h.update(seed, len);
    uint8_t d[64];
    h.finish(d);
    uint64_t v[4];
    fs_to_uniform(d, 64, v);
    memcpy(spending_key_out, v, 32);
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_jubjub_base_mul(const uint8_t* scalars, size_t n, uint8_t* points_out) try {
    if (n && (!scalars || !points_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    (void)zkwit::tables();
    // test hook (tests/test_gen_proof.py): the LAST worker thread fails an allocation - the exception must reach the caller as
    // a status, through run_threads and the barrier of this entry, not unwind into it
    const bool inject = hook_env("ZKAMD_INJECT_THROW") != nullptr;
    return for_each_status(n, 64, [&](size_t i) -> zk_status {
        if (inject && i + 1 == n) throw std::bad_alloc();
        uint64_t k[4];
        load_scalar_le(scalars + 32 * i, k);
        if (!fs_lt_mod(k)) return fail(ZK_ERR_INVALID_ARGUMENT, "scalar " + std::to_string(i) + " is not a canonical Fs scalar");
        const zkwit::JPoint p = jubjub_fixed_mul(k);
        jubjub_encode(p.x, p.y, points_out + 32 * i);
        return ZK_OK;
    });
} ZK_ABI_CATCH

zk_status zk_elgamal_encrypt(const uint32_t* values, const uint8_t* randomness, const uint8_t* enc_keys, size_t n, uint8_t* left_out,
                             uint8_t* right_out) try {
    if (n && (!values || !randomness || !enc_keys || !left_out || !right_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    (void)zkwit::tables();
    return for_each_status(n, 16, [&](size_t i) -> zk_status {
        uint64_t r[4], v[4] = {values[i], 0, 0, 0};
        load_scalar_le(randomness + 32 * i, r);
        zkwit::JPoint key;
        if (!fs_lt_mod(r)) return fail(ZK_ERR_INVALID_ARGUMENT, "randomness " + std::to_string(i) + " is not a canonical Fs scalar");
        ZK_TRY(decode_prime_order(enc_keys + 32 * i, &key, "enc_key " + std::to_string(i)));
        // left = v G + r pk, right = r G  (no_std_aliases/elgamal.rs:46-63)
        zkwit::EPoint proj[2] = {zkwit::ext_add(zkwit::to_ext(jubjub_fixed_mul(v)), jubjub_var_mul(key, r)), zkwit::to_ext(jubjub_fixed_mul(r))};
        zkwit::JPoint aff[2];
        zkwit::batch_to_affine(proj, aff, 2);
        jubjub_encode(aff[0].x, aff[0].y, left_out + 32 * i);
        jubjub_encode(aff[1].x, aff[1].y, right_out + 32 * i);
        return ZK_OK;
    });
} ZK_ABI_CATCH

// ElGamal decryption (elgamal.rs:85-108) as a baby-step giant-step search: the table and the search are witness.cpp's
// (kernels: elgamal_dlog.h); the point work of every ciphertext - decoding, dk * right - stays on host threads here.
zk_status zk_elgamal_table_create(uint32_t baby_bits, int device, zk_elgamal_table** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const uint32_t b = baby_bits ? baby_bits : ELGAMAL_BABY_BITS_DEFAULT;
    if (b < ELGAMAL_BABY_BITS_MIN || b > ELGAMAL_BABY_BITS_MAX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "baby_bits " + std::to_string(baby_bits) + " is outside 8 .. 24");
    ZK_TRY(use_device(device));
    std::unique_ptr<zk_elgamal_table> t(new zk_elgamal_table());
    t->device = device;
    t->baby_bits = b;
    // test hook (tests/test_elgamal_decrypt.py): a narrower fingerprint, so that most probes hit slots of other points
    if (const char* e = hook_env("ZKAMD_DEBUG_DLOG_FP_BITS")) t->fp_bits = (uint32_t)std::min(32, std::max(0, atoi(e)));
    ZK_TRY(elgamal_table_build(t.get()));
    *out = t.release();
    return ZK_OK;
} ZK_ABI_CATCH

void zk_elgamal_table_free(zk_elgamal_table* t) {
    if (!t) return;
    try {
        (void)use_device(t->device);   // the buffers go back (the key-derived ones zeroed) on the handle's device
    } catch (...) {
    }
    delete t;
}

zk_status zk_elgamal_decrypt(zk_elgamal_table* t, size_t n, const uint8_t* left, const uint8_t* right, const uint8_t* dec_keys,
                             size_t dec_key_stride, uint64_t limit, uint32_t* values_out, uint8_t* found_out) try {
    if (!t || (n && (!left || !right || !dec_keys || !values_out || !found_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (dec_key_stride != 0 && dec_key_stride != 32)
        return fail(ZK_ERR_INVALID_ARGUMENT, "dec_key_stride must be 0 (one key for all) or 32 (one key per ciphertext)");
    ZK_TRY(zkscan::check_limit(limit));
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(t->device));
    // v = left - dk right (elgamal.rs:92-94), affine: the value is its logarithm
    std::vector<zkwit::JPoint> v(n);
    WipeOnExit wipe_v{v.data(), n * sizeof(zkwit::JPoint)};
    ZK_TRY(for_each_range(n, 16, [&](size_t i0, size_t i1) -> zk_status {
        std::vector<zkwit::EPoint> proj(i1 - i0);
        WipeOnExit wipe_p{proj.data(), proj.size() * sizeof(zkwit::EPoint)};
        for (size_t i = i0; i < i1; i++) {
            uint64_t dk[4];
            WipeOnExit wipe_dk{dk, sizeof(dk)};
            load_scalar_le(dec_keys + dec_key_stride * i, dk);
            const std::string who = "ciphertext " + std::to_string(i) + ": ";
            zkwit::JPoint l, r;
            if (!fs_lt_mod(dk))
                return fail(ZK_ERR_INVALID_ARGUMENT, (dec_key_stride ? "dec_key " + std::to_string(i) : std::string("dec_key")) + " is not a canonical Fs scalar");
            ZK_TRY(decode_prime_order(left + 32 * i, &l, who + "left"));
            ZK_TRY(decode_prime_order(right + 32 * i, &r, who + "right"));
            const zkwit::EPoint s = jubjub_var_mul(r, dk);
            proj[i - i0] = zkwit::ext_add(zkwit::to_ext(l), zkwit::EPoint{zkhost::Fr::zero() - s.X, s.Y, s.Z, zkhost::Fr::zero() - s.T});
        }
        zkwit::batch_to_affine(proj.data(), v.data() + i0, i1 - i0);
        return ZK_OK;
    }));
    std::vector<uint64_t> x(n);
    WipeOnExit wipe_x{x.data(), n * sizeof(uint64_t)};
    static_assert(sizeof(zkwit::JPoint) == 2 * sizeof(zkhost::Fr), "x | y");
    ZK_TRY(elgamal_dlog_search(t, n, &v[0].x, limit, x.data()));
    for (size_t i = 0; i < n; i++) {
        const bool found = x[i] < limit;   // (the search reports ~0 for none)
        values_out[i] = found ? (uint32_t)x[i] : 0u;
        found_out[i] = found ? 1 : 0;
    }
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_confidential_scan(zk_elgamal_table* t, size_t n, const zk_confidential_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                               zk_confidential_scan_result* out) try {
    return zkscan::scan<zkscan::Confidential>(t, n, xts, dec_key, limit, out);
} ZK_ABI_CATCH

zk_status zk_anonymous_scan(zk_elgamal_table* t, size_t n, const zk_anonymous_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                            zk_anonymous_scan_result* out) try {
    return zkscan::scan<zkscan::Anonymous>(t, n, xts, dec_key, limit, out);
} ZK_ABI_CATCH

zk_status zk_scan_keys_create(const uint8_t* dec_keys, size_t n_keys, zk_scan_keys** out) try {
    return zkscan::keys_create(dec_keys, n_keys, out);
} ZK_ABI_CATCH

zk_status zk_scan_keys_get(const zk_scan_keys* k, size_t first, size_t count, uint8_t* enc_keys_out) try {
    return zkscan::keys_get(k, first, count, enc_keys_out);
} ZK_ABI_CATCH

void zk_scan_keys_free(zk_scan_keys* k) {
    delete k;   // (the scalars are wiped by the destructor)
}

zk_status zk_confidential_scan_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n, const zk_confidential_xt* xts, uint64_t limit,
                                    zk_confidential_scan_hit* hits_out, size_t hits_cap, size_t* n_hits_out) try {
    return zkscan::scan_keys<zkscan::Confidential>(t, keys, n, xts, limit, hits_out, hits_cap, n_hits_out);
} ZK_ABI_CATCH

zk_status zk_anonymous_scan_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n, const zk_anonymous_xt* xts, uint64_t limit,
                                 zk_anonymous_scan_hit* hits_out, size_t hits_cap, size_t* n_hits_out) try {
    return zkscan::scan_keys<zkscan::Anonymous>(t, keys, n, xts, limit, hits_out, hits_cap, n_hits_out);
} ZK_ABI_CATCH

zk_status zk_balance_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n_accounts, const zk_block_account* accounts, uint64_t limit,
                          zk_balance_hit* hits_out, size_t hits_cap, size_t* n_hits_out) try {
    return zkscan::balance_keys(t, keys, n_accounts, accounts, limit, hits_out, hits_cap, n_hits_out);
} ZK_ABI_CATCH

zk_status zk_hd_master(const uint8_t* seed, size_t len, uint8_t xsk_out[73]) try {
    if ((!seed && len) || !xsk_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return zkhd::master(seed, len, xsk_out);
} ZK_ABI_CATCH

zk_status zk_hd_xpgk_from_xsk(const uint8_t xsk[73], uint8_t xpgk_out[73]) try {
    if (!xsk || !xpgk_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return zkhd::xpgk_from_xsk(xsk, xpgk_out);
} ZK_ABI_CATCH

zk_status zk_hd_derive(uint32_t kind, const uint8_t xkey[73], const uint32_t* indices, size_t n, int device, uint8_t* xkeys_out,
                       uint8_t* dec_keys_out, uint8_t* enc_keys_out) try {
    return zkhd::derive(kind, xkey, indices, n, device, xkeys_out, dec_keys_out, enc_keys_out);
} ZK_ABI_CATCH

zk_status zk_scan_keys_create_hd(uint32_t kind, const uint8_t xkey[73], const uint32_t* indices, size_t n, int device, zk_scan_keys** out) try {
    return zkhd::scan_keys_create(kind, xkey, indices, n, device, out);
} ZK_ABI_CATCH

zk_status zk_jubjub_base_mul_dev(const uint8_t* scalars, const uint8_t* addends, size_t n, int device, uint8_t* points_out,
                                 uint8_t* status_out) try {
    return zkhd::base_mul_dev(scalars, addends, n, device, points_out, status_out);
} ZK_ABI_CATCH

zk_status zk_elgamal_add(const uint8_t* left_a, const uint8_t* right_a, const uint8_t* left_b, const uint8_t* right_b, size_t n,
                         int subtract, uint8_t* left_out, uint8_t* right_out) try {
    if (n && (!left_a || !right_a || !left_b || !right_b || !left_out || !right_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    return for_each_status(n, 16, [&](size_t i) -> zk_status {
        // Ciphertext::read of both operands (elgamal.rs:116-133), then left_a +- left_b, right_a +- right_b
        const uint8_t* in[4] = {left_a + 32 * i, right_a + 32 * i, left_b + 32 * i, right_b + 32 * i};
        static const char* const name[4] = {"left_a", "right_a", "left_b", "right_b"};
        zkwit::JPoint p[4];
        for (int k = 0; k < 4; k++) ZK_TRY(decode_prime_order(in[k], &p[k], "ciphertext " + std::to_string(i) + ": " + name[k]));
        if (subtract) {
            p[2].x = zkhost::Fr::zero() - p[2].x;
            p[3].x = zkhost::Fr::zero() - p[3].x;
        }
        const zkwit::EPoint sum[2] = {zkwit::ext_add(zkwit::to_ext(p[0]), zkwit::to_ext(p[2])), zkwit::ext_add(zkwit::to_ext(p[1]), zkwit::to_ext(p[3]))};
        zkwit::JPoint aff[2];
        zkwit::batch_to_affine(sum, aff, 2);
        jubjub_encode(aff[0].x, aff[0].y, left_out + 32 * i);
        jubjub_encode(aff[1].x, aff[1].y, right_out + 32 * i);
        return ZK_OK;
    });
} ZK_ABI_CATCH

zk_status zk_transfer_derive(const zk_transfer_request* req, size_t n, zk_transfer_statement* statements_out, uint8_t* rsk_out) try {
    if (n && (!req || !statements_out || !rsk_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return transfer_derive(req, n, statements_out, rsk_out, true);
} ZK_ABI_CATCH

}  // extern "C"
extern "C" {

zk_status zk_transfer_gen_proof_batch(zk_params* p, zk_r1cs* circuit, zk_vk* vk, size_t n, const zk_transfer_request* req,
                                      const uint8_t* rs, zk_confidential_xt* out) try {
    if (!p || !circuit || !vk || (n && (!req || !rs || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(p, circuit, 0, n));
    if (n == 0) return ZK_OK;
    std::vector<zk_transfer_statement> st(n);
    std::vector<uint8_t> rsk(n * 32), proofs(n * 192), ok(n);
    WipeOnExit wipe_st{st.data(), n * sizeof(zk_transfer_statement)}, wipe_rsk{rsk.data(), rsk.size()};
    // ZKAMD_DEBUG_TIMING=1: where the wall time of the call goes (stderr)
    const bool timing = hook_env("ZKAMD_DEBUG_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    // A handful of requests (one transaction at a time is the reference's call pattern): the assignment on the host cores,
    // 1.4 ms per statement, instead of the witness kernels' 8.4 ms of serial chains (statement_route.h witness_on_host); the typed
    // inputs are then checked here, otherwise by the witness kernels of the chunk.
    const bool host_wit = lib_witness_on_host(n);
    ZK_TRY(transfer_derive(req, n, st.data(), rsk.data(), host_wit));
    if (timing) fprintf(stderr, "[gen_proof] derive done %.1f ms\n", since());
    const size_t n_pub = ZK_TRANSFER_N_INPUTS - 1;
    std::vector<uint8_t> inputs(n * n_pub * 32);
    // the prover leaves the affine A, B, C of every proof here for the self-check below (host_common.h g_own_affine_sink)
    std::vector<uint8_t> own_aff(n * OWN_AFFINE_BYTES);
    OwnAffineSink sink(own_aff.data());
    size_t n_chunks = 0;
    // the proofs chunk by chunk, the witnesses of the next chunk beside the proving of this one (zkamd.cpp lib_transfer_chunks); as
    // each is proved, its statements' 23 public inputs (heads) are packed with the proofs
    ZK_TRY(lib_transfer_chunks(p, circuit, n, st.data(), rs, proofs.data(), [&](size_t first, size_t np, const uint8_t* heads, size_t head_stride) {
        if (timing) fprintf(stderr, "[gen_proof] chunk %zu proved %.1f ms\n", n_chunks, since());
        n_chunks++;
        for (size_t i = 0; i < np; i++) {
            const zkhost::Fr* z = reinterpret_cast<const zkhost::Fr*>(heads + i * head_stride);
            zk_confidential_xt& x = out[first + i];
            memset(&x, 0, sizeof(x));
            for (size_t k = 0; k < n_pub; k++) {
                const zkhost::Fr pl = z[1 + k].from_mont();
                memcpy(&inputs[((first + i) * n_pub + k) * 32], pl.l, 32);
            }
            memcpy(x.proof, proofs.data() + (first + i) * 192, 192);
            jubjub_encode(z[1], z[2], x.enc_key_sender);
            jubjub_encode(z[3], z[4], x.enc_key_recipient);
            jubjub_encode(z[5], z[6], x.left_amount_sender);
            jubjub_encode(z[7], z[8], x.left_amount_recipient);
            jubjub_encode(z[9], z[10], x.right_randomness);
            jubjub_encode(z[11], z[12], x.left_fee);
            jubjub_encode(z[13], z[14], x.enc_balance);
            jubjub_encode(z[15], z[16], x.enc_balance + 32);
            jubjub_encode(z[17], z[18], x.rvk);
            jubjub_encode(z[21], z[22], x.nonce);
            memcpy(x.rsk, rsk.data() + (first + i) * 32, 32);
        }
        return ZK_OK;
    }, timing ? &t_start : nullptr));
    // check_proof of every proof of the call, in ONE set of launches at the end: a verification is a bundle of serial
    // chains (a few hundred waves on the whole GPU) whose duration hardly depends on how many proofs it holds - 8.0 ms for
    // 1024, 9.2 for 2048 (round 2: 45 ms).  Run beside the proving of the next chunk, as rounds 2 and 3 first did, it is
    // starved by the persistent accumulation launches (its one-wave-per-SIMD kernels wait for a whole SIMD's
    // registers): chunk 0's check was still running 335 ms later and the call waited 40 ms for it
    // (profiles/r03_experiments.txt r03q).
    if (timing) fprintf(stderr, "[gen_proof] packed %.1f ms\n", since());
    ZK_TRY(verify_batch(vk, n, proofs.data(), inputs.data(), n_pub, ok.data(), true, VERIFY_AUTO, own_aff.data()));
    if (timing) fprintf(stderr, "[gen_proof] done %.1f ms\n", since());
    for (size_t i = 0; i < n; i++)
        if (!ok[i]) return fail(ZK_ERR_UNSATISFIABLE, "request " + std::to_string(i) + ": the proof does not verify (inconsistent statement)");
    return ZK_OK;
} ZK_ABI_CATCH

// ------------------------------------------------------------------------------------------
// gen_proof of the anonymous transfer (core/proofs/src/anonymous.rs:97-183, 267-352): the same derivations, the
// anonymity set assembled around the sender and the recipient, MultiCiphertexts::<Anonymous>::encrypt
// (crypto_components.rs:168-220: the sender's amount negated, the recipient's positive, zero under every decoy key,
// one randomness), check_proof over the 104 public coordinates (:213-264) and the packing of AnonymousXt.
// ------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

struct AnonDerived {
    zkwit::JPoint pub[4 * ZK_ANONYMOUS_SIZE + 4];   // the public points in the order of the circuit's inputs
};

zk_status anonymous_derive_one(const zk_anonymous_request& rq, size_t index, zk_anonymous_statement* st, uint8_t rsk[32],
                               AnonDerived* der) {
    const std::string who = "request " + std::to_string(index) + ": ";
    if (rq.s_index >= ZK_ANONYMOUS_SIZE || rq.t_index >= ZK_ANONYMOUS_SIZE || rq.s_index == rq.t_index)
        return fail(ZK_ERR_INVALID_ARGUMENT, who + "s_index and t_index must be two different members of the set");
    uint64_t sk[4], alpha[4], rnd[4], dk[4] = {0, 0, 0, 0};
    WipeOnExit wipe_sk{sk, sizeof(sk)}, wipe_alpha{alpha, sizeof(alpha)}, wipe_rnd{rnd, sizeof(rnd)}, wipe_dk{dk, sizeof(dk)};   // every exit path
    load_scalar_le(rq.spending_key, sk);
    load_scalar_le(rq.alpha, alpha);
    load_scalar_le(rq.randomness, rnd);
    if (!fs_lt_mod(sk)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "spending_key is not a canonical Fs scalar");
    if (!fs_lt_mod(alpha)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "alpha is not a canonical Fs scalar");
    if (!fs_lt_mod(rnd)) return fail(ZK_ERR_INVALID_ARGUMENT, who + "randomness is not a canonical Fs scalar");
    memset(st, 0, sizeof(*st));
    st->amount = rq.amount;
    st->remaining_balance = rq.remaining_balance;
    st->s_index = rq.s_index;
    st->t_index = rq.t_index;
    memcpy(st->randomness, rq.randomness, 32);
    memcpy(st->alpha, rq.alpha, 32);
    memcpy(st->g_epoch, rq.g_epoch, 32);
    const zkwit::JPoint pgk = jubjub_fixed_mul(sk);
    jubjub_encode(pgk.x, pgk.y, st->proof_generation_key);
    static const uint8_t person[8] = {'z', 'e', 'c', 'h', '_', 'b', 'd', 'k'};
    zkhash::Blake2s h(person);
    h.update(st->proof_generation_key, 32);
    h.finish(st->dec_key);
    st->dec_key[31] &= 0x07;
    load_scalar_le(st->dec_key, dk);
    // the set: sender at s_index, recipient at t_index, the decoys in their order everywhere else
    zkwit::JPoint keys[ZK_ANONYMOUS_SIZE];
    keys[rq.s_index] = jubjub_fixed_mul(dk);
    ZK_TRY(decode_prime_order(rq.enc_key_recipient, &keys[rq.t_index], who + "enc_key_recipient"));
    for (size_t i = 0, j = 0; i < ZK_ANONYMOUS_SIZE; i++) {
        if (i == rq.s_index || i == rq.t_index) continue;
        ZK_TRY(decode_prime_order(rq.enc_keys_decoy[j], &keys[i], who + "enc_keys_decoy[" + std::to_string(j) + "]"));
        j++;
    }
    zkwit::JPoint g_epoch;
    ZK_TRY(decode_prime_order(rq.g_epoch, &g_epoch, who + "g_epoch"));
    for (size_t i = 0; i < ZK_ANONYMOUS_SIZE; i++) {
        const std::string m = "[" + std::to_string(i) + "]";
        ZK_TRY(decode_prime_order(rq.enc_balances_left[i], nullptr, who + "enc_balances_left" + m));
        ZK_TRY(decode_prime_order(rq.enc_balances_right[i], nullptr, who + "enc_balances_right" + m));
    }
    // left ciphertexts v_i G + r y_i, right r G, rvk = pgk + alpha G, nonce = dec_key * g_epoch: one batch to affine
    uint64_t amt[4] = {rq.amount, 0, 0, 0};
    const zkwit::JPoint amount_g = jubjub_fixed_mul(amt);
    const zkwit::JPoint neg_amount_g{zkhost::Fr::zero() - amount_g.x, amount_g.y};
    zkwit::EPoint proj[ZK_ANONYMOUS_SIZE + 3];
    for (size_t i = 0; i < ZK_ANONYMOUS_SIZE; i++) {
        proj[i] = jubjub_var_mul(keys[i], rnd);
        if (i == rq.s_index) proj[i] = zkwit::ext_add(proj[i], zkwit::to_ext(neg_amount_g));
        if (i == rq.t_index) proj[i] = zkwit::ext_add(proj[i], zkwit::to_ext(amount_g));
    }
    proj[ZK_ANONYMOUS_SIZE] = zkwit::to_ext(jubjub_fixed_mul(rnd));
    proj[ZK_ANONYMOUS_SIZE + 1] = zkwit::ext_add(zkwit::to_ext(pgk), zkwit::to_ext(jubjub_fixed_mul(alpha)));
    proj[ZK_ANONYMOUS_SIZE + 2] = jubjub_var_mul(g_epoch, dk);
    zkwit::JPoint aff[ZK_ANONYMOUS_SIZE + 3];
    zkwit::batch_to_affine(proj, aff, ZK_ANONYMOUS_SIZE + 3);
    for (size_t i = 0; i < ZK_ANONYMOUS_SIZE; i++) {
        jubjub_encode(keys[i].x, keys[i].y, st->enc_keys[i]);
        jubjub_encode(aff[i].x, aff[i].y, st->left_ciphertexts[i]);
        memcpy(st->enc_balances_left[i], rq.enc_balances_left[i], 32);
        memcpy(st->enc_balances_right[i], rq.enc_balances_right[i], 32);
    }
    uint64_t r[4];
    WipeOnExit wipe_r{r, sizeof(r)};
    fs_add(sk, alpha, r);   // SpendingKey::into_rsk
    memcpy(rsk, r, 32);
    if (der) {
        for (size_t i = 0; i < ZK_ANONYMOUS_SIZE; i++) {
            der->pub[i] = keys[i];
            der->pub[ZK_ANONYMOUS_SIZE + i] = aff[i];
            const std::string m = "[" + std::to_string(i) + "] is not a Jubjub point";
            if (!zkwit::decode_point(rq.enc_balances_left[i], &der->pub[2 * ZK_ANONYMOUS_SIZE + i]))
                return fail(ZK_ERR_INVALID_ARGUMENT, who + "enc_balances_left" + m);
            if (!zkwit::decode_point(rq.enc_balances_right[i], &der->pub[3 * ZK_ANONYMOUS_SIZE + i]))
                return fail(ZK_ERR_INVALID_ARGUMENT, who + "enc_balances_right" + m);
        }
        der->pub[4 * ZK_ANONYMOUS_SIZE] = aff[ZK_ANONYMOUS_SIZE];           // right ciphertext
        der->pub[4 * ZK_ANONYMOUS_SIZE + 1] = aff[ZK_ANONYMOUS_SIZE + 1];   // rvk
        der->pub[4 * ZK_ANONYMOUS_SIZE + 2] = g_epoch;
        der->pub[4 * ZK_ANONYMOUS_SIZE + 3] = aff[ZK_ANONYMOUS_SIZE + 2];   // nonce
    }
    return ZK_OK;
}
zk_status anonymous_derive(const zk_anonymous_request* rq, size_t n, zk_anonymous_statement* st, uint8_t* rsk, AnonDerived* der) {
    if (n == 0) return ZK_OK;
    (void)zkwit::tables();
    return for_each_status(n, 8, [&](size_t i) -> zk_status { return anonymous_derive_one(rq[i], i, &st[i], rsk + i * 32, der ? &der[i] : nullptr); });
}

}  // namespace

#include "anon_derive.h"    // (the same derivation with a device form: its lanes through derive_stage.h's point kernel and combine)
#include "elgamal_encrypt.h"   // (encryption under many keys with a device form: its lanes through the same two kernels)

extern "C" {

zk_status zk_elgamal_encrypt_dev(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys, int device,
                                 uint8_t* left_out, uint8_t* right_out, uint8_t* status_out) try {
    return zkenc::encrypt(n, k, values, randomness, enc_keys, device, left_out, right_out, status_out);
} ZK_ABI_CATCH

zk_status zk_anonymous_derive(const zk_anonymous_request* req, size_t n, zk_anonymous_statement* statements_out, uint8_t* rsk_out) try {
    if (n && (!req || !statements_out || !rsk_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return anonymous_derive(req, n, statements_out, rsk_out, nullptr);
} ZK_ABI_CATCH

zk_status zk_anonymous_derive_dev(const zk_anonymous_request* req, size_t n, int device, zk_anonymous_statement* statements_out, uint8_t* rsk_out,
                                  uint8_t* inputs_out) try {
    if (n == 0) return ZK_OK;
    if (!req || !statements_out || !rsk_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return zkanon::derive(req, n, device, statements_out, rsk_out, inputs_out, nullptr);
} ZK_ABI_CATCH

zk_status zk_anonymous_gen_proof_batch(zk_params* p, zk_r1cs* circuit, zk_vk* vk, size_t n, const zk_anonymous_request* req,
                                       const uint8_t* rs, zk_anonymous_xt* out) try {
    if (!p || !circuit || !vk || (n && (!req || !rs || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    const size_t n_pub = zkanon::N_PUB;
    std::vector<zk_anonymous_statement> st(n);
    std::vector<uint8_t> rsk(n * 32), proofs(n * 192), ok(n), inputs(n * n_pub * 32), tail(n * 96);
    WipeOnExit wipe_st{st.data(), n * sizeof(zk_anonymous_statement)}, wipe_rsk{rsk.data(), rsk.size()};
    // the statements, the 104 coordinates of check_proof and the three points the statement does not carry, from the one stage
    // (anon_derive.h), on the circuit's device - the key's too, or zk_anonymous_prove_batch refuses the pair
    ZK_TRY(zkanon::derive(req, n, circuit->sys.device, st.data(), rsk.data(), inputs.data(), tail.data()));
    ZK_TRY(zk_anonymous_prove_batch(p, circuit, n, st.data(), rs, proofs.data()));
    for (size_t i = 0; i < n; i++) {
        zk_anonymous_xt& x = out[i];
        memset(&x, 0, sizeof(x));
        memcpy(x.proof, &proofs[i * 192], 192);
        memcpy(x.enc_keys, st[i].enc_keys, sizeof(x.enc_keys));
        memcpy(x.left_ciphertexts, st[i].left_ciphertexts, sizeof(x.left_ciphertexts));
        memcpy(x.right_ciphertext, &tail[96 * i], 32);
        memcpy(x.rvk, &tail[96 * i + 32], 32);
        memcpy(x.nonce, &tail[96 * i + 64], 32);
        memcpy(x.rsk, &rsk[i * 32], 32);
    }
    // check_proof (anonymous.rs:213-264)
    ZK_TRY(verify_batch(vk, n, proofs.data(), inputs.data(), n_pub, ok.data(), true));
    for (size_t i = 0; i < n; i++)
        if (!ok[i]) return fail(ZK_ERR_UNSATISFIABLE, "request " + std::to_string(i) + ": the proof does not verify (inconsistent statement)");
    return ZK_OK;
} ZK_ABI_CATCH

}  // extern "C"
