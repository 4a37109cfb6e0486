// A block's transfers read with a SET of decryption keys in one call (zk_scan_keys_*, zk_confidential_scan_keys,
// zk_anonymous_scan_keys): every pair (extrinsic, key of the set) in which the extrinsic carries the key, with the result the
// single-key entry writes for that key.  The reference has no counterpart; the parts are those of elgamal_scan.h.
// Included by wallet.cpp below elgamal_scan.h (zkscan::Plan, Keys, run), and by no other unit.
//
// The handle derives the K encryption keys once, on the zk_set_host_threads pool, and keeps an index from their 32 bytes to the
// key's number.  A call matches every extrinsic against that index on the host - a hit is one (extrinsic, key) - and then runs
// the plan of elgamal_scan.h with one match per hit: the same points, rows and search rows the single-key entry builds for that
// key.  What changes is the point stage's multiplier: dk * right takes the scalar of the HIT - jubjub_var_mul once per hit in the
// host form, k_keys_points (wallet_stage.h) in the place of k_scan_points in the device form, with the per-hit scalars (H x 32
// bytes, gathered from the handle) as the head.  Nothing of the key set stays on the device between calls.
#pragma once
#include "elgamal_scan.h"

struct zk_scan_keys {
    std::vector<uint64_t> dk;      // n x 4 words, plain
    std::vector<uint8_t> enc;      // n x 32 bytes: EncryptionKey::from_decryption_key of each
    std::vector<uint32_t> order;   // the key numbers sorted by those bytes
    size_t n() const { return order.size(); }
    zkscan::Keys view() const { return zkscan::Keys{n(), dk.data(), enc.data(), order.data()}; }
    ~zk_scan_keys() {
        if (!dk.empty()) explicit_bzero(dk.data(), dk.size() * sizeof(uint64_t));
    }
};

namespace zkscan {

// The two halves of a key set's construction, shared by zk_scan_keys_create and zk_scan_keys_create_hd (hd_keys.h), which differ in
// where the encryption keys come from.  keys_load: the handle with its n_keys canonical scalars and room for their encryption keys.
inline zk_status keys_load(const uint8_t* dec_keys, size_t n_keys, std::unique_ptr<zk_scan_keys>* out) {
    if (n_keys == 0 || n_keys > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, "n_keys must be 1 .. 2^32 - 1");
    std::unique_ptr<zk_scan_keys> k(new zk_scan_keys());
    k->dk.resize(n_keys * 4);
    k->enc.resize(n_keys * 32);
    for (size_t i = 0; i < n_keys; i++) {
        zkrt::load_scalar_le(dec_keys + 32 * i, &k->dk[4 * i]);
        if (!fs_lt_mod(&k->dk[4 * i])) return fail(ZK_ERR_INVALID_ARGUMENT, "dec_key " + std::to_string(i) + " is not a canonical Fs scalar");
    }
    *out = std::move(k);
    return ZK_OK;
}
// keys_index: with k->enc filled, the sort by those bytes, the duplicate check and the handle's release to the caller
inline zk_status keys_index(std::unique_ptr<zk_scan_keys> k, zk_scan_keys** out) {
    const size_t n_keys = k->enc.size() / 32;
    k->order.resize(n_keys);
    for (size_t i = 0; i < n_keys; i++) k->order[i] = (uint32_t)i;
    const uint8_t* enc = k->enc.data();
    std::sort(k->order.begin(), k->order.end(), [enc](uint32_t a, uint32_t b) {
        const int c = memcmp(enc + 32 * (size_t)a, enc + 32 * (size_t)b, 32);
        return c ? c < 0 : a < b;
    });
    // s is prime and every scalar below it: two keys have the same bytes exactly when their scalars are equal
    for (size_t i = 0; i + 1 < n_keys; i++)
        if (!memcmp(enc + 32 * (size_t)k->order[i], enc + 32 * (size_t)k->order[i + 1], 32))
            return fail(ZK_ERR_INVALID_ARGUMENT, "dec_key " + std::to_string(k->order[i]) + " and dec_key " + std::to_string(k->order[i + 1]) + " are equal");
    *out = k.release();
    return ZK_OK;
}
inline zk_status keys_create(const uint8_t* dec_keys, size_t n_keys, zk_scan_keys** out) {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (!dec_keys) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_ptr<zk_scan_keys> k;
    ZK_TRY(keys_load(dec_keys, n_keys, &k));
    (void)zkwit::tables();
    ZK_TRY(zkrt::for_each_status(n_keys, 64, [&](size_t i) -> zk_status {
        const zkwit::JPoint pk = jubjub_fixed_mul(&k->dk[4 * i]);   // EncryptionKey::from_decryption_key
        jubjub_encode(pk.x, pk.y, &k->enc[32 * i]);
        return ZK_OK;
    }));
    return keys_index(std::move(k), out);
}

inline zk_status keys_get(const zk_scan_keys* k, size_t first, size_t count, uint8_t* enc_keys_out) {
    if (!k || (count && !enc_keys_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (first > k->n() || count > k->n() - first)
        return fail(ZK_ERR_INVALID_ARGUMENT, "keys " + std::to_string(first) + " .. + " + std::to_string(count) + " are outside the set of " + std::to_string(k->n()));
    if (count) memcpy(enc_keys_out, &k->enc[32 * first], 32 * count);
    return ZK_OK;
}

// The cap-and-count contract of the key-set entries.  count(keys): the hits, before any other work.  More than hits_cap: the count is
// reported and nothing is written.  Else hits_out[0 .. count) is zeroed and run(keys, count) fills it; a half-written array does
// not leave the call.  too_many, of_what: the entry's words for n of 2^32 or more, and for its input in the hits_cap message.
template <class HitOut, class Count, class Run>
inline zk_status with_hits(zk_elgamal_table* t, const zk_scan_keys* k, size_t n, const void* items, uint64_t limit, const char* too_many, const char* of_what,
                           HitOut* hits_out, size_t hits_cap, size_t* n_hits_out, Count count, Run run) {
    if (!t || !k || !n_hits_out || (n && !items)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(check_limit(limit));
    *n_hits_out = 0;
    if (n == 0) return ZK_OK;
    if (n > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, too_many);
    const Keys keys = k->view();
    const size_t total = count(keys);
    if (total > hits_cap) {
        *n_hits_out = total;
        return fail(ZK_ERR_INVALID_ARGUMENT, "hits_cap " + std::to_string(hits_cap) + " is below the " + std::to_string(total) + " hits of " + of_what);
    }
    if (total == 0) return ZK_OK;
    if (!hits_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(zkrt::use_device(t->device));
    memset(hits_out, 0, total * sizeof(HitOut));
    const zk_status rc = run(keys, total);
    if (rc != ZK_OK) {
        explicit_bzero(hits_out, total * sizeof(HitOut));
        return rc;
    }
    *n_hits_out = total;
    return ZK_OK;
}

// hits_out[h]: the h-th hit in (xt, key) order.  Matching runs twice: once to count and once to plan.
template <class Kind, class HitOut>
inline zk_status scan_keys(zk_elgamal_table* t, const zk_scan_keys* k, size_t n, const typename Kind::Xt* xts, uint64_t limit, HitOut* hits_out,
                           size_t hits_cap, size_t* n_hits_out) {
    return with_hits(
        t, k, n, xts, limit, "a hit numbers its extrinsic in 32 bits: n must be below 2^32", "this block", hits_out, hits_cap, n_hits_out,
        [&](const Keys& keys) -> size_t {
            Hit hits[MAX_HITS_PER_XT];
            size_t total = 0;
            for (size_t i = 0; i < n; i++) total += Kind::match(xts[i], keys, hits);
            return total;
        },
        [&](const Keys& keys, size_t) -> zk_status {
            return run<Kind>(t, keys, n, xts, limit, [hits_out](size_t h, size_t xt, uint32_t key) {
                hits_out[h].xt = (uint32_t)xt;
                hits_out[h].key = key;
                return &hits_out[h].r;
            });
        });
}

}  // namespace zkscan
