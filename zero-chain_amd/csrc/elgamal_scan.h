// A block's transfers read with ONE decryption key (zk_confidential_scan, zk_anonymous_scan): which extrinsics touch the key,
// and by how much.  The reference has no counterpart; the pieces are EncryptionKey::from_decryption_key (keys.rs:250-261) for
// the match, Ciphertext::read (elgamal.rs:116-133) for the points the wallet's role uses, Ciphertext::decrypt (elgamal.rs:85-108)
// for every value, and the signs of MultiCiphertexts::<Anonymous>::encrypt (crypto_components.rs:168-220).
// Included by wallet.cpp below wallet_stage.h (the point stage: device_stage, HostRows, the point kernels), and by no other unit.
// The host side below serves a SET of keys as well (scan_keys.h): a match carries the number of its key (always 0 here), the plan,
// the host form and the slicing are shared, and only the multiplier of the point kernel differs.
//
// The host matches the 32 bytes of the wallet's key against the keys of every extrinsic and gathers, for the matching ones only,
//   points   every used left half and the right half, in the push order of the verifiers' field numbers
//   rights   the right half again, once per matching extrinsic: dk * right is shared by all its values
//   rows     one per value to decrypt: (left point, right point, right)
// and the point stage (wallet_stage.h) brings every row to v = left - dk right.  An anonymous row is searched twice, as v and as
// -v: the sender's ciphertext holds -amount.  Its two forms here:
//   host    zkwit::decode_point + is_prime_order, jubjub_var_mul once per match, then HostRows
//   device  k_scan_points (one key: the width-4 NAF of dk) or k_keys_points (a set: the scalar of every match), then
//     k_scan_combine  one lane per row: v = left - D (one addition), to affine form by one inversion, stored as two Montgomery
//                     Fr straight into the table's v buffer (and -v behind it for an anonymous row).  A row whose left or right
//                     half was refused stores the neutral element and raises its flag: the host ignores what the search finds.
#pragma once
#include "wallet_stage.h"

namespace zkscan {

// field numbers of zk_confidential_verify_batch / zk_anonymous_verify_batch
enum { F_LEFT_AMOUNT_SENDER = 3, F_LEFT_AMOUNT_RECIPIENT = 4, F_RIGHT_RANDOMNESS = 5, F_LEFT_FEE = 6, F_LEFT_CIPHERTEXTS = 13, F_RIGHT_CIPHERTEXT = 49 };

// rows: n_rows x 4 words - left point, right point, right, first search row | ROW_ANON.  xy, status: the point kernel's of the
// points, d_in its d_out.  v: the table's buffer (zkdlog::Search::v: per search row x then y, Montgomery).  flags: n_rows words.
static __global__ void __launch_bounds__(64)
k_scan_combine(const uint32_t* rows, uint32_t n_rows, const uint32_t* xy, const uint32_t* status, const uint32_t* d_in, uint32_t* v,
               uint32_t* flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_rows) return;
    const uint4 row = reinterpret_cast<const uint4*>(rows)[i];
    const bool refused = status[row.x] != zkxt::INTO_XY_OK || status[row.y] != zkxt::INTO_XY_OK;
    Fr x = Fr::zero(), y = Fr::one();
    if (!refused) {
        const Fr lx = zkrj::ld_fr(xy + (size_t)row.x * 16), ly = zkrj::ld_fr(xy + (size_t)row.x * 16 + 8);
        const uint32_t* dd = d_in + (size_t)row.z * 32;
        const EP minus_d{neg(zkrj::ld_fr(dd)), zkrj::ld_fr(dd + 8), zkrj::ld_fr(dd + 16), neg(zkrj::ld_fr(dd + 24))};
        const EP s = zkxt::ext_add(EP{lx, ly, Fr::one(), mul(lx, ly)}, minus_d, zkxt::jubjub_d2());
        const uint32_t rm2[8] = ZK_FR_EXP_RM2_32;
        const Fr zi = zkdev::pow_limbs(s.Z, rm2);   // (Z != 0: the addition law is complete on the prime-order subgroup)
        x = mul(s.X, zi);
        y = mul(s.Y, zi);
    }
    uint32_t* o = v + (size_t)(row.w & ~ROW_ANON) * 16;
    st_fr(o, x);
    st_fr(o + 8, y);
    if (row.w & ROW_ANON) {
        st_fr(o + 16, neg(x));
        st_fr(o + 24, y);
    }
    flags[i] = refused ? 1u : 0u;
}

// ---- host side
struct Row {
    uint32_t left, right_pt, right, out;   // point indices, the index among the rights, the first search row | ROW_ANON
};
struct Match {
    size_t xt;             // index of the extrinsic in the caller's array
    uint32_t pt0, row0;    // its points and rows start here and end where the next match's start
    uint32_t key;          // the number of the key it matched (0 where the call has one key)
};
// The decryption keys of a call: ONE (zk_confidential_scan, zk_anonymous_scan) or a set (scan_keys.h).  A match carries the number
// of its key, and the point stage multiplies its right half by that key's scalar.
struct Keys {
    size_t n;
    const uint64_t* dk;      // n x 4 words, plain
    const uint8_t* enc;      // n x 32 bytes: EncryptionKey::from_decryption_key of each
    const uint32_t* order;   // the key numbers sorted by those bytes (memcmp order); NULL for the one key of zk_*_scan
    const uint64_t* scalar(uint32_t k) const { return dk + 4 * (size_t)k; }
    // the number of the key whose 32 bytes are b, or -1
    int64_t find(const uint8_t b[32]) const {
        if (!order) return memcmp(b, enc, 32) ? -1 : 0;
        size_t lo = 0, hi = n;
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            const int c = memcmp(enc + 32 * (size_t)order[mid], b, 32);
            if (c == 0) return order[mid];
            (c < 0 ? lo : hi) = c < 0 ? mid + 1 : mid;
        }
        return -1;
    }
};
// one (key, mask) per key of the call that an extrinsic carries, by key number: mask = role bits (confidential), members (anonymous)
struct Hit {
    uint32_t key, mask;
};
constexpr size_t MAX_HITS_PER_XT = 12;   // ZK_ANONYMOUS_SIZE keys in a ring, all of the set
// what one slice of a call decrypts: at most ELGAMAL_SEARCH_BLOCK search rows
struct Plan {
    std::vector<Match> matches;
    std::vector<uint8_t> enc, field;   // per point: 32 bytes, its field number
    std::vector<Row> rows;
    std::vector<uint8_t> what;         // per row, the caller's: which value (confidential) or which member (anonymous)
    uint32_t n_search = 0;
    size_t points() const { return field.size(); }
    uint32_t point(const uint8_t* e, uint8_t f) {
        enc.insert(enc.end(), e, e + 32);
        field.push_back(f);
        return (uint32_t)field.size() - 1;
    }
    void row(uint32_t left, uint32_t right_pt, uint8_t w, bool anon) {
        rows.push_back(Row{left, right_pt, (uint32_t)matches.size() - 1, n_search | (anon ? ROW_ANON : 0u)});
        what.push_back(w);
        n_search += anon ? 2 : 1;
    }
    void close() { matches.push_back(Match{(size_t)-1, (uint32_t)points(), (uint32_t)rows.size(), 0}); }   // the end marker
};
// what the point stage and the search leave: a status per point, a flag per row, a logarithm (or ~0) per search row
struct Found {
    std::vector<uint8_t> status;
    std::vector<uint32_t> flags;
    std::vector<uint64_t> x;
    void wipe() {
        if (!x.empty()) explicit_bzero(x.data(), x.size() * sizeof(uint64_t));
    }
    ~Found() { wipe(); }
};

// the width-4 NAF of k < 2^252, zkxt::digits_order's recoding at run time
inline void naf_recode(const uint64_t k_in[4], uint8_t out[DIGITS_BYTES]) {
    uint64_t k[4] = {k_in[0], k_in[1], k_in[2], k_in[3]};
    WipeOnExit wipe_k{k, sizeof(k)};
    memset(out, 0, DIGITS_BYTES);
    int32_t top = -1;
    for (int i = 0; i < 256; i++) {
        if (k[0] & 1u) {
            int v = (int)(k[0] & 15u);
            if (v >= 8) v -= 16;
            out[i] = (uint8_t)(int8_t)v;
            top = i;
            if (v > 0) {
                k[0] -= (uint64_t)v;
            } else {
                const uint64_t a = (uint64_t)(-v), old = k[0];
                k[0] += a;
                if (k[0] < old)
                    for (int j = 1; j < 4 && ++k[j] == 0; j++) {}
            }
        }
        for (int j = 0; j < 4; j++) k[j] = (k[j] >> 1) | (j < 3 ? k[j + 1] << 63 : 0);
    }
    memcpy(out + 256, &top, 4);
}

// Point::read + as_prime_order of one encoding, as zk_jubjub_into_xy's host form decides it
inline uint8_t read_prime_order(const uint8_t b[32], zkwit::JPoint* out) {
    uint64_t v[4];
    zkrt::load_scalar_le(b, v);
    v[3] &= 0x7fffffffffffffffull;
    if (zkhost::Fr::geq_p(v)) return zkxt::INTO_XY_NOT_IN_FIELD;
    if (!zkwit::decode_point(b, out)) return zkxt::INTO_XY_NOT_ON_CURVE;
    if (!zkwit::is_prime_order(*out)) return zkxt::INTO_XY_NOT_PRIME_ORDER;
    return zkxt::INTO_XY_OK;
}

inline void launch_scan_combine(const StageBufs& B) {
    ZK_LAUNCH(k_scan_combine, B.row_grid(), dim3(64), 0, zkrt::g_stream, B.rows, B.n_rows, (const uint32_t*)B.xy, (const uint32_t*)B.status,
              (const uint32_t*)B.d, B.v, B.flags);
}
const StageKernel SCAN_COMBINE{"scan_combine", launch_scan_combine};

// the host form: the statuses, the flags, and v of every search row into T->v
inline zk_status points_on_host(zk_elgamal_table* T, const Plan& pl, const Keys& keys, Found* f) {
    HostRows hr(pl.n_search);
    ZK_TRY(zkrt::for_each_range(pl.matches.size() - 1, 64, [&](size_t m0, size_t m1) -> zk_status {
        const uint32_t r0 = pl.matches[m0].row0, r1 = pl.matches[m1].row0;
        std::vector<zkwit::EPoint> proj(r1 - r0, zkwit::ext_zero());
        std::vector<zkwit::JPoint> aff(r1 - r0), pts;
        WipeOnExit wipe_p{proj.data(), proj.size() * sizeof(zkwit::EPoint)}, wipe_a{aff.data(), aff.size() * sizeof(zkwit::JPoint)};
        for (size_t m = m0; m < m1; m++) {
            const Match &a = pl.matches[m], &b = pl.matches[m + 1];
            pts.resize(b.pt0 - a.pt0);
            bool ok = true;
            for (uint32_t p = a.pt0; p < b.pt0; p++) ok &= (f->status[p] = read_prime_order(&pl.enc[(size_t)p * 32], &pts[p - a.pt0])) == zkxt::INTO_XY_OK;
            for (uint32_t r = a.row0; r < b.row0; r++)
                f->flags[r] = f->status[pl.rows[r].left] != zkxt::INTO_XY_OK || f->status[pl.rows[r].right_pt] != zkxt::INTO_XY_OK;
            if (!ok) continue;   // a refused extrinsic: its rows stay the neutral element
            const zkwit::EPoint s = jubjub_var_mul(pts[pl.rows[a.row0].right_pt - a.pt0], keys.scalar(a.key));
            const zkwit::EPoint minus_s{zkhost::Fr::zero() - s.X, s.Y, s.Z, zkhost::Fr::zero() - s.T};
            for (uint32_t r = a.row0; r < b.row0; r++) proj[r - r0] = zkwit::ext_add(zkwit::to_ext(pts[pl.rows[r].left - a.pt0]), minus_s);
        }
        hr.land(proj, aff, 0, 1, [&](size_t k) { return pl.rows[r0 + k].out; });
        return ZK_OK;
    }));
    return hr.upload(T);
}

// the device form: the same three.  One key (keys.order == NULL): its width-4 NAF, recoded here once per call, and k_scan_points;
// a set: the scalar of every match, gathered for this slice, and k_keys_points
inline zk_status points_on_device(zk_elgamal_table* T, const Plan& pl, const Keys& keys, Found* f) {
    const size_t nm = pl.matches.size() - 1;
    std::vector<uint8_t> rights(nm * 32), head(keys.order ? nm * 32 : DIGITS_BYTES);
    WipeOnExit wipe_head{head.data(), head.size()};
    static_assert(sizeof(uint64_t[4]) == 32 && sizeof(Row) == 16, "eight plain words, little-endian; four words");
    for (size_t m = 0; m < nm; m++) {
        memcpy(&rights[m * 32], &pl.enc[(size_t)pl.rows[pl.matches[m].row0].right_pt * 32], 32);
        if (keys.order) memcpy(&head[m * 32], keys.scalar(pl.matches[m].key), 32);
    }
    if (!keys.order) naf_recode(keys.scalar(0), head.data());
    const Slice s{pl.enc, rights, head, pl.rows.data(), pl.rows.size(), 16, 4, pl.n_search, keys.order ? KEYS_POINTS : SCAN_POINTS, SCAN_COMBINE};
    return device_stage(T, s, f->flags.data(), f->status.data());
}

// one slice: the point stage in the form the row count asks for, then the search over the rows resident in T->v
inline zk_status decrypt_plan(zk_elgamal_table* T, Plan& pl, const Keys& keys, uint64_t limit, Found* f) {
    pl.close();
    f->status.assign(pl.points(), 0);
    f->flags.assign(pl.rows.size(), 0);
    f->x.assign(pl.n_search, ~0ull);
    if (pl.rows.empty()) return ZK_OK;
    ZK_TRY((pl.rows.size() <= host_max() ? points_on_host : points_on_device)(T, pl, keys, f));
    return elgamal_dlog_search_resident(T, pl.n_search, limit, f->x.data());
}
// field | status << 6 of the first refused point of match m in push order, or 0
inline uint8_t refusal_of(const Plan& pl, const Found& f, size_t m) {
    for (uint32_t p = pl.matches[m].pt0; p < pl.matches[m + 1].pt0; p++)
        if (f.status[p]) return (uint8_t)(pl.field[p] | f.status[p] << 6);
    return 0;
}

// The two kinds of extrinsic share everything but how one is matched and how its rows are read back:
//   match(xt, keys, hits)            the keys of the call that xt carries, by key number, each with its mask; returns their count
//   add(plan, xt, index, hit)        pushes the match of one of them, its points and its rows
//   finish(plan, found, m, limit, out)   writes the result of match m
struct Confidential {
    typedef zk_confidential_xt Xt;
    typedef zk_confidential_scan_result Result;
    static constexpr size_t ROWS_PER_XT = 3;   // search rows of one extrinsic, over all its matches
    static size_t match(const Xt& x, const Keys& keys, Hit hits[MAX_HITS_PER_XT]) {
        const int64_t s = keys.find(x.enc_key_sender), r = keys.find(x.enc_key_recipient);
        size_t n = 0;
        if (s >= 0 && s == r) {
            hits[n++] = Hit{(uint32_t)s, ZK_SCAN_SENDER | ZK_SCAN_RECIPIENT};   // a transfer to oneself
        } else {
            if (s >= 0) hits[n++] = Hit{(uint32_t)s, ZK_SCAN_SENDER};
            if (r >= 0) hits[n++] = Hit{(uint32_t)r, ZK_SCAN_RECIPIENT};
            if (n == 2 && hits[0].key > hits[1].key) std::swap(hits[0], hits[1]);
        }
        return n;
    }
    static void add(Plan& pl, const Xt& x, size_t i, const Hit& h) {
        const bool s = h.mask & ZK_SCAN_SENDER, r = h.mask & ZK_SCAN_RECIPIENT;
        pl.matches.push_back(Match{i, (uint32_t)pl.points(), (uint32_t)pl.rows.size(), h.key});
        const uint32_t ls = s ? pl.point(x.left_amount_sender, F_LEFT_AMOUNT_SENDER) : 0, lr = r ? pl.point(x.left_amount_recipient, F_LEFT_AMOUNT_RECIPIENT) : 0;
        const uint32_t right = pl.point(x.right_randomness, F_RIGHT_RANDOMNESS), lf = s ? pl.point(x.left_fee, F_LEFT_FEE) : 0;
        if (s) pl.row(ls, right, ZK_SCAN_FOUND_SENT, false);
        if (s) pl.row(lf, right, ZK_SCAN_FOUND_FEE, false);
        if (r) pl.row(lr, right, ZK_SCAN_FOUND_RECEIVED, false);
    }
    static void finish(const Plan& pl, const Found& f, size_t m, uint64_t limit, Result* o) {
        const Match &a = pl.matches[m], &b = pl.matches[m + 1];
        for (uint32_t r = a.row0; r < b.row0; r++) o->role |= pl.what[r] == ZK_SCAN_FOUND_RECEIVED ? ZK_SCAN_RECIPIENT : ZK_SCAN_SENDER;
        if ((o->refusal = refusal_of(pl, f, m)) != 0) return;
        for (uint32_t r = a.row0; r < b.row0; r++) {
            const uint64_t x = f.x[pl.rows[r].out];
            if (f.flags[r] || x >= limit) continue;   // (the search reports ~0 for none)
            o->found |= pl.what[r];
            (pl.what[r] == ZK_SCAN_FOUND_SENT ? o->amount_sent : pl.what[r] == ZK_SCAN_FOUND_FEE ? o->fee : o->amount_received) = (uint32_t)x;
        }
    }
};
struct Anonymous {
    typedef zk_anonymous_xt Xt;
    typedef zk_anonymous_scan_result Result;
    static constexpr size_t ROWS_PER_XT = 2 * ZK_ANONYMOUS_SIZE;
    static_assert(ZK_ANONYMOUS_SIZE <= MAX_HITS_PER_XT, "one hit per member at the most");
    static size_t match(const Xt& x, const Keys& keys, Hit hits[MAX_HITS_PER_XT]) {
        size_t n = 0;
        for (uint32_t k = 0; k < ZK_ANONYMOUS_SIZE; k++) {
            const int64_t key = keys.find(x.enc_keys[k]);
            if (key < 0) continue;
            size_t at = 0;
            while (at < n && hits[at].key < (uint32_t)key) at++;
            if (at == n || hits[at].key != (uint32_t)key) {
                for (size_t j = n++; j > at; j--) hits[j] = hits[j - 1];
                hits[at] = Hit{(uint32_t)key, 0};
            }
            hits[at].mask |= 1u << k;
        }
        return n;
    }
    static void add(Plan& pl, const Xt& x, size_t i, const Hit& h) {
        const uint32_t members = h.mask;
        pl.matches.push_back(Match{i, (uint32_t)pl.points(), (uint32_t)pl.rows.size(), h.key});
        uint32_t left[ZK_ANONYMOUS_SIZE];
        for (uint32_t k = 0; k < ZK_ANONYMOUS_SIZE; k++)
            if (members >> k & 1) left[k] = pl.point(x.left_ciphertexts[k], (uint8_t)(F_LEFT_CIPHERTEXTS + k));
        const uint32_t right = pl.point(x.right_ciphertext, F_RIGHT_CIPHERTEXT);
        for (uint32_t k = 0; k < ZK_ANONYMOUS_SIZE; k++)
            if (members >> k & 1) pl.row(left[k], right, (uint8_t)k, true);
    }
    static void finish(const Plan& pl, const Found& f, size_t m, uint64_t limit, Result* o) {
        const Match &a = pl.matches[m], &b = pl.matches[m + 1];
        for (uint32_t r = a.row0; r < b.row0; r++) o->members |= (uint16_t)(1u << pl.what[r]);
        if ((o->refusal = refusal_of(pl, f, m)) != 0) return;
        int64_t delta = 0;
        for (uint32_t r = a.row0; r < b.row0; r++) {
            const uint32_t s = pl.rows[r].out & ~ROW_ANON;
            const uint64_t plus = f.x[s], minus = f.x[s + 1];   // x G == v, x G == -v (both for x = 0)
            if (f.flags[r] || (plus >= limit && minus >= limit)) return;   // one occurrence without a value: found stays 0
            delta += plus < limit ? (int64_t)plus : -(int64_t)minus;
        }
        o->found = 1;
        o->delta = delta;
    }
};

// Every match of the block, slice by slice (at most ELGAMAL_SEARCH_BLOCK search rows each):
//   slot(h, xt, key)                 where the result of match h - counted over the whole call, in (xt, key) order - goes; zeroed
template <class Kind, class Slot>
inline zk_status run(zk_elgamal_table* t, const Keys& keys, size_t n, const typename Kind::Xt* xts, uint64_t limit, Slot slot) {
    Plan pl;
    Found f;
    size_t done = 0;
    auto flush = [&]() -> zk_status {
        ZK_TRY(decrypt_plan(t, pl, keys, limit, &f));
        for (size_t m = 0; m + 1 < pl.matches.size(); m++) Kind::finish(pl, f, m, limit, slot(done + m, pl.matches[m].xt, pl.matches[m].key));
        done += pl.matches.size() - 1;
        f.wipe();
        pl = Plan();
        return ZK_OK;
    };
    Hit hits[MAX_HITS_PER_XT];
    for (size_t i = 0; i < n; i++) {
        if (pl.n_search + Kind::ROWS_PER_XT > ELGAMAL_SEARCH_BLOCK) ZK_TRY(flush());
        const size_t nh = Kind::match(xts[i], keys, hits);
        for (size_t h = 0; h < nh; h++) Kind::add(pl, xts[i], i, hits[h]);
    }
    return flush();
}

// one key: out[i] is the result of extrinsic i, all zero where it does not carry the key
template <class Kind>
inline zk_status scan(zk_elgamal_table* t, size_t n, const typename Kind::Xt* xts, const uint8_t dec_key[32], uint64_t limit, typename Kind::Result* out) {
    if (!t || (n && (!xts || !dec_key || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(check_limit(limit));
    if (n == 0) return ZK_OK;
    uint64_t dk[4];
    WipeOnExit wipe_dk{dk, sizeof(dk)};
    zkrt::load_scalar_le(dec_key, dk);
    if (!fs_lt_mod(dk)) return fail(ZK_ERR_INVALID_ARGUMENT, "dec_key is not a canonical Fs scalar");
    ZK_TRY(zkrt::use_device(t->device));
    uint8_t key[32];
    {
        const zkwit::JPoint pk = jubjub_fixed_mul(dk);   // EncryptionKey::from_decryption_key
        jubjub_encode(pk.x, pk.y, key);
    }
    memset(out, 0, n * sizeof(typename Kind::Result));
    return run<Kind>(t, Keys{1, dk, key, nullptr}, n, xts, limit, [out](size_t, size_t xt, uint32_t) { return &out[xt]; });
}

}  // namespace zkscan
