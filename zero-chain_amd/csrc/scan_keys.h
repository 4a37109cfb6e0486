// A block's transfers read with a SET of decryption keys in one call (zk_scan_keys_*, zk_confidential_scan_keys,
// zk_anonymous_scan_keys): every pair (extrinsic, key of the set) in which the extrinsic carries the key, with the result the
// single-key entry writes for that key.  The reference has no counterpart; the parts are those of elgamal_scan.h:
// EncryptionKey::from_decryption_key (keys.rs:250-261), Ciphertext::decrypt (elgamal.rs:85-108) and the signs of
// MultiCiphertexts::<Anonymous>::encrypt (crypto_components.rs:168-220).
// Included by wallet.cpp below elgamal_scan.h (zkscan::Plan, Keys, run, points_on_device, k_scan_combine), and by no other unit.
//
// The handle derives the K encryption keys once, on the zk_set_host_threads pool, and keeps an index from their 32 bytes to the
// key's number.  A call matches every extrinsic against that index on the host - a hit is one (extrinsic, key) - and then runs
// the plan of elgamal_scan.h with one match per hit: the same points, rows and search rows the single-key entry builds for that
// key.  What changes is the point stage: dk * right takes the scalar of the HIT.
//   host    jubjub_var_mul once per hit (points_on_host, the match's key)
//   device  k_keys_points in the place of k_scan_points, then k_scan_combine and the search as they are
//     k_keys_points   one wave per block, two kinds of lane split at a wave boundary
//                       lanes [0, P)          k_scan_points' first kind: read_point + is_prime_order, one status word per point
//                       lanes [P64, P64 + H)  one per hit: read_point of the hit's right half, then D = [dk_hit] right with the
//                                             lane's OWN scalar.  A NAF would put every lane's additions at its own positions,
//                                             so the chain is k_rj_check's: signed FIXED windows of W = 3 bits (booth_digit,
//                                             read off the scalar's words in an LDS slot), three doublings per window and one
//                                             ext_add_cached against 1 .. 4 times right where the digit is not zero - all 64
//                                             lanes add at the same 85 positions.
//                                               252 doublings (8 products)                                 2 016
//                                               up to 85 additions of a cached multiple (8 products)         680
//                                               the four cached multiples (a doubling, two additions, 4 x 1)  ~30
//                                             after read_point's ~620: about 3 350 dependent products, against ~3 000 of the
//                                             single-key lane (620 + 252 doublings + ~50 additions of its NAF).
//                     LDS, [slot][word][lane]: slots 0 .. 15 the window table of read_point / is_prime_order, then the cached
//                     multiples (Y + X, Y - X, 2 d T, 2 Z) of 1 .. 4 times right; slot 16 the eight plain words of the lane's
//                     scalar (dynamic indexing of registers would go to scratch) = 17 x 32 x 64 = 34 816 B, nothing in scratch.
// Secrets: the per-hit scalars, D, v and the logarithms are key-derived.  The scalars travel per call in the head of the table's
// scan_key buffer (H x 32 bytes, gathered from the handle) with D behind them, v in the table's v buffer; both are zeroed on the
// device after every call and on every failure path, the host copies wiped on every way out.  Nothing of the key set stays on
// the device between calls.  The device form is NOT constant-time: a zero digit skips its addition, so the lanes' paths depend on
// the scalars; the host form multiplies with jubjub_var_mul, whose steps do not depend on them.
#pragma once
#include "elgamal_scan.h"

struct zk_scan_keys {
    std::vector<uint64_t> dk;      // n x 4 words, plain
    std::vector<uint8_t> enc;      // n x 32 bytes: EncryptionKey::from_decryption_key of each
    std::vector<uint32_t> order;   // the key numbers sorted by those bytes
    size_t n() const { return order.size(); }
    ~zk_scan_keys() {
        if (!dk.empty()) explicit_bzero(dk.data(), dk.size() * sizeof(uint64_t));
    }
};

namespace zkscan {

constexpr int KEYS_WINDOW = 3, KEYS_MULTIPLES = 1 << (KEYS_WINDOW - 1);
constexpr uint32_t KEYS_SLOT_SCALAR = 16, KEYS_LDS_SLOTS = 17, KEYS_LDS_BYTES = KEYS_LDS_SLOTS * 32 * 64;
static_assert(252 % KEYS_WINDOW == 0, "the last window at bit 252 holds bit 251 alone");
static_assert(4 * KEYS_MULTIPLES <= (int)KEYS_SLOT_SCALAR && KEYS_LDS_BYTES <= 36864, "the cached multiples below the scalar, in k_rj_check's budget");

// enc, xy, status: as k_scan_points.  enc_right: n_hits x 8 words.  scalars: n_hits x 8 plain words, the scalar of each hit.
// d_out: n_hits x 32 words, X Y Z T of [scalar] right (the neutral element where the encoding is no point: kind 1 reports it).
static __global__ void __launch_bounds__(64)
k_keys_points(const uint32_t* enc, uint32_t n_points, uint32_t p64, const uint32_t* enc_right, uint32_t n_hits, const uint32_t* scalars,
              uint32_t* xy, uint32_t* status, uint32_t* d_out) {
    ZK_SHARED uint32_t table[KEYS_LDS_SLOTS * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    const Lds L{table + threadIdx.x};
    Fr x = Fr::zero(), y, xm = Fr::zero(), ym = Fr::zero(), d;
    if (t < p64) {
        if (t >= n_points) return;
        uint32_t st = zkxt::read_point(L, enc + (size_t)t * 8, &x, &y, &xm, &ym, &d);
        if (st == zkxt::INTO_XY_OK && !zkxt::is_prime_order(L, xm, ym, dbl(d))) st = zkxt::INTO_XY_NOT_PRIME_ORDER;
        if (st != zkxt::INTO_XY_OK) xm = ym = Fr::zero();
        st_fr(xy + (size_t)t * 16, xm);
        st_fr(xy + (size_t)t * 16 + 8, ym);
        status[t] = st;
    } else {
        const uint32_t r = t - p64;
        if (r >= n_hits) return;
        EP acc{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
        if (zkxt::read_point(L, enc_right + (size_t)r * 8, &x, &y, &xm, &ym, &d) == zkxt::INTO_XY_OK) {
            L.st(KEYS_SLOT_SCALAR, zkrj::ld_fr(scalars + (size_t)r * 8));
            const Fr d2 = dbl(d);
            {   // right, 2 right .. in slots 4 i .. 4 i + 3
                EP q{xm, ym, Fr::one(), mul(xm, ym)};
                zkxt::cache_put(L, 0, q, d2);
                q = zkxt::ext_dbl(q, true);
                zkxt::cache_put(L, 1, q, d2);
#pragma unroll 1
                for (uint32_t i = 2; i < (uint32_t)KEYS_MULTIPLES; i++) {
                    q = zkxt::ext_add_cached(L, q, 0, false, true);
                    zkxt::cache_put(L, i, q, d2);
                }
            }
#pragma unroll 1
            for (int j = 252 / KEYS_WINDOW; j >= 0; j--) {
                if (j != 252 / KEYS_WINDOW) {
#pragma unroll
                    for (int k = 0; k < KEYS_WINDOW - 1; k++) acc = zkxt::ext_dbl(acc, false);
                    acc = zkxt::ext_dbl(acc, true);
                }
                const int dv = zkrj::booth_digit<KEYS_WINDOW>(L, KEYS_SLOT_SCALAR, (uint32_t)(KEYS_WINDOW * j));
                if (dv) acc = zkxt::ext_add_cached(L, acc, (uint32_t)((dv < 0 ? -dv : dv) - 1), dv < 0, true);
            }
        }
        uint32_t* o = d_out + (size_t)r * 32;
        st_fr(o, acc.X);
        st_fr(o + 8, acc.Y);
        st_fr(o + 16, acc.Z);
        st_fr(o + 24, acc.T);
    }
}

// ---- host side
// a set of keys: the scalar of every match, gathered for this slice, and k_keys_points
inline zk_status points_per_hit(zk_elgamal_table* T, const Plan& pl, const Keys& keys, Found* f) {
    const size_t nm = pl.matches.size() - 1;
    std::vector<uint8_t> scalars(nm * 32);
    WipeOnExit wipe_scalars{scalars.data(), scalars.size()};
    static_assert(sizeof(uint64_t[4]) == 32, "eight plain words, little-endian");
    for (size_t m = 0; m < nm; m++) memcpy(&scalars[m * 32], keys.scalar(pl.matches[m].key), 32);
    return points_on_device(T, pl, scalars, f, [](dim3 grid, const uint32_t* enc, uint32_t np, uint32_t p64, const uint32_t* right, uint32_t nm, void* head,
                                                  uint32_t* xy, uint32_t* status, uint32_t* d) {
        zkrt::ProfScope ps("keys_points");
        ZK_LAUNCH(k_keys_points, grid, dim3(64), 0, zkrt::g_stream, enc, np, p64, right, nm, (const uint32_t*)head, xy, status, d);
    });
}

inline zk_status keys_create(const uint8_t* dec_keys, size_t n_keys, zk_scan_keys** out) {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (!dec_keys) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n_keys == 0 || n_keys > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, "n_keys must be 1 .. 2^32 - 1");
    std::unique_ptr<zk_scan_keys> k(new zk_scan_keys());
    k->dk.resize(n_keys * 4);
    k->enc.resize(n_keys * 32);
    for (size_t i = 0; i < n_keys; i++) {
        zkrt::load_scalar_le(dec_keys + 32 * i, &k->dk[4 * i]);
        if (!fs_lt_mod(&k->dk[4 * i])) return fail(ZK_ERR_INVALID_ARGUMENT, "dec_key " + std::to_string(i) + " is not a canonical Fs scalar");
    }
    (void)zkwit::tables();
    const unsigned nth = zkrt::host_threads(n_keys, 64);
    auto work = [&](unsigned th) {
        for (size_t i = n_keys * th / nth; i < n_keys * (th + 1) / nth; i++) {
            const zkwit::JPoint pk = jubjub_fixed_mul(&k->dk[4 * i]);   // EncryptionKey::from_decryption_key
            jubjub_encode(pk.x, pk.y, &k->enc[32 * i]);
        }
    };
    zkrt::run_threads(nth, work);
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

inline zk_status keys_get(const zk_scan_keys* k, size_t first, size_t count, uint8_t* enc_keys_out) {
    if (!k || (count && !enc_keys_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (first > k->n() || count > k->n() - first)
        return fail(ZK_ERR_INVALID_ARGUMENT, "keys " + std::to_string(first) + " .. + " + std::to_string(count) + " are outside the set of " + std::to_string(k->n()));
    if (count) memcpy(enc_keys_out, &k->enc[32 * first], 32 * count);
    return ZK_OK;
}

// hits_out[h]: the h-th hit in (xt, key) order.  Matching runs twice: once to count, before any other work, and once to plan.
template <class Kind, class HitOut>
inline zk_status scan_keys(zk_elgamal_table* t, const zk_scan_keys* k, size_t n, const typename Kind::Xt* xts, uint64_t limit, HitOut* hits_out,
                           size_t hits_cap, size_t* n_hits_out) {
    if (!t || !k || !n_hits_out || (n && !xts)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (limit == 0 || limit > (1ull << 32)) return fail(ZK_ERR_INVALID_ARGUMENT, "limit must be 1 .. 2^32");
    *n_hits_out = 0;
    if (n == 0) return ZK_OK;
    if (n > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, "a hit numbers its extrinsic in 32 bits: n must be below 2^32");
    const Keys keys{k->n(), k->dk.data(), k->enc.data(), k->order.data()};
    size_t total = 0;
    {
        Hit hits[MAX_HITS_PER_XT];
        for (size_t i = 0; i < n; i++) total += Kind::match(xts[i], keys, hits);
    }
    if (total > hits_cap) {
        *n_hits_out = total;
        return fail(ZK_ERR_INVALID_ARGUMENT, "hits_cap " + std::to_string(hits_cap) + " is below the " + std::to_string(total) + " hits of this block");
    }
    if (total == 0) return ZK_OK;
    if (!hits_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(zkrt::use_device(t->device));
    memset(hits_out, 0, total * sizeof(HitOut));
    const zk_status rc = run<Kind>(t, keys, n, xts, limit, points_per_hit, [hits_out](size_t h, size_t xt, uint32_t key) {
        hits_out[h].xt = (uint32_t)xt;
        hits_out[h].key = key;
        return &hits_out[h].r;
    });
    if (rc != ZK_OK) {   // a half-written array does not leave the call
        explicit_bzero(hits_out, total * sizeof(HitOut));
        return rc;
    }
    *n_hits_out = total;
    return ZK_OK;
}

}  // namespace zkscan
