// A block's transfers read with ONE decryption key (zk_confidential_scan, zk_anonymous_scan): which extrinsics touch the key,
// and by how much.  The reference has no counterpart; the pieces are EncryptionKey::from_decryption_key (keys.rs:250-261) for
// the match, Ciphertext::read (elgamal.rs:116-133) for the points the wallet's role uses, Ciphertext::decrypt (elgamal.rs:85-108)
// for every value, and the signs of MultiCiphertexts::<Anonymous>::encrypt (crypto_components.rs:168-220).
// Included by wallet.cpp below redjubjub.h (fs_lt_mod, jubjub_fixed_mul, jubjub_var_mul, jubjub_encode, WipeOnExit, zkrj::ld_fr).
// The host side below serves a SET of keys as well (scan_keys.h): a match carries the number of its key (always 0 here), the plan,
// the host form and the slicing are shared, and only the kernel that multiplies differs.
//
// The host matches the 32 bytes of the wallet's key against the keys of every extrinsic and gathers, for the matching ones only,
//   points   every used left half and the right half, in the push order of the verifiers' field numbers
//   rights   the right half again, once per matching extrinsic: dk * right is shared by all its values
//   rows     one per value to decrypt: (left point, right point, right)
// and then brings every row to v = left - dk right, affine, in the table's v buffer, where the search of zk_elgamal_decrypt
// (witness.cpp elgamal_dlog_search_resident) finds the logarithms.  An anonymous row is searched twice, as v and as -v: the
// sender's ciphertext holds -amount.  Two forms of the point work, the same bytes:
//   host    zkwit::decode_point + is_prime_order, jubjub_var_mul once per extrinsic and batch_to_affine on the
//           zk_set_host_threads pool, one upload of v
//   device  two launches on the library stream, one wave per block:
//     k_scan_points   one lane per task, the two kinds split at a wave boundary (the point count is padded to 64)
//                       lanes [0, P)          read_point + is_prime_order: k_into_xy's body, the coordinates left in Montgomery form
//                       lanes [P64, P64 + R)  read_point of a right half, then D = [dk] right over the width-4 NAF of dk, recoded
//                                             on the host once per call: 252 doublings and an addition per non-zero digit against
//                                             +-R, +-3R, +-5R, +-7R cached in LDS - is_prime_order's steps and its chain length.
//                                             Every lane reads the same digits, so a wave takes one path.
//                     LDS as k_into_xy: [slot][word][lane], 16 slots, 32 768 B per block, nothing in scratch memory.
//     k_scan_combine  one lane per row: v = left - D (one addition), to affine form by one inversion, stored as two Montgomery
//                     Fr straight into the table's v buffer (and -v behind it for an anonymous row).  A row whose left or right
//                     half was refused stores the neutral element and raises its flag: the host ignores what the search finds.
// Secrets: the digits of dk, D, v and the logarithms are key-derived - their device buffers are zeroed after every call and
// before release, the host copies wiped on every way out.  The encodings, coordinates and statuses are public chain data.
// The device form is NOT constant-time: the digits of dk decide where the shared chain adds, as the bits of the keys decide the
// shape of the witness kernels' chains today; the host form multiplies with jubjub_var_mul, whose steps do not depend on dk.
#pragma once
#include "redjubjub.h"
#include "handles.h"

namespace zkscan {

using zkdev::Fr;
using zkrt::fail;
using zkxt::EP;
using zkxt::Lds;

// ZKAMD_SCAN_HOST_MAX: rows (values to decrypt) up to which the host form runs.  Measured (profiles/r14_scan_probe.json, 16 host
// threads, recipient rows at limit 10^6): the device form is 2.85 - 2.95 ms from 64 to 1024 rows, the host form 2.45 ms at 128 rows
// and 4.60 ms at 256 - 128 is the largest probed size at which the host form is still the faster one.
constexpr size_t HOST_MAX = 128;
// (read per call; zk_balance_keys counts its hits against the same value, balance_keys.h)
inline size_t host_max() {
    const char* e = getenv("ZKAMD_SCAN_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
}
constexpr uint32_t ROW_ANON = 1u << 31;       // in a row's fourth word: also store -v, one search row further
constexpr size_t DIGITS_BYTES = 272;          // 256 digits, their top index as an int32, padded to 16 bytes
// field numbers of zk_confidential_verify_batch / zk_anonymous_verify_batch
enum { F_LEFT_AMOUNT_SENDER = 3, F_LEFT_AMOUNT_RECIPIENT = 4, F_RIGHT_RANDOMNESS = 5, F_LEFT_FEE = 6, F_LEFT_CIPHERTEXTS = 13, F_RIGHT_CIPHERTEXT = 49 };

ZK_DI void st_fr(uint32_t* p, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// enc: p64 x 8 words (n_points of them used).  xy: n_points x 16 words, x then y in Montgomery form, zero where refused.  status:
// n_points words, zkxt::INTO_XY_*.  enc_right: n_rights x 8 words.  digits: 256 signed digits, then their top index (int32).
// d_out: n_rights x 32 words, X Y Z T of [dk] right (the neutral element where the encoding is no point: kind 1 reports it).
static __global__ void __launch_bounds__(64)
k_scan_points(const uint32_t* enc, uint32_t n_points, uint32_t p64, const uint32_t* enc_right, uint32_t n_rights, const int8_t* digits,
              uint32_t* xy, uint32_t* status, uint32_t* d_out) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
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
        if (r >= n_rights) return;
        EP acc{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
        if (zkxt::read_point(L, enc_right + (size_t)r * 8, &x, &y, &xm, &ym, &d) == zkxt::INTO_XY_OK)
            acc = zkxt::mul_naf(L, xm, ym, dbl(d), digits, *reinterpret_cast<const int32_t*>(digits + 256));
        uint32_t* o = d_out + (size_t)r * 32;
        st_fr(o, acc.X);
        st_fr(o + 8, acc.Y);
        st_fr(o + 16, acc.Z);
        st_fr(o + 24, acc.T);
    }
}

// rows: n_rows x 4 words - left point, right point, right, first search row | ROW_ANON.  xy, status: k_scan_points' of the points,
// d_in its d_out.  v: the table's buffer (zkdlog::Search::v: per search row x then y, Montgomery).  flags: n_rows words.
static __global__ void __launch_bounds__(64)
k_scan_combine(const uint32_t* rows, uint32_t n_rows, const uint32_t* xy, const uint32_t* status, const uint32_t* d_in, uint32_t* v,
               uint32_t* flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_rows) return;
    const uint4 row = reinterpret_cast<const uint4*>(rows)[i];
    const bool refused = status[row.x] != zkxt::INTO_XY_OK || status[row.y] != zkxt::INTO_XY_OK;
    Fr x = Fr::zero(), y = Fr::one();
    if (!refused) {
        Fr d;
        {
            const uint64_t dp[4] = ZK_JUBJUB_D_PLAIN_64;
#pragma unroll
            for (int k = 0; k < 8; k++) d.l[k] = (uint32_t)(dp[k >> 1] >> (32 * (k & 1)));
        }
        const Fr lx = zkrj::ld_fr(xy + (size_t)row.x * 16), ly = zkrj::ld_fr(xy + (size_t)row.x * 16 + 8);
        const uint32_t* dd = d_in + (size_t)row.z * 32;
        const EP minus_d{neg(zkrj::ld_fr(dd)), zkrj::ld_fr(dd + 8), zkrj::ld_fr(dd + 16), neg(zkrj::ld_fr(dd + 24))};
        const EP s = zkxt::ext_add(EP{lx, ly, Fr::one(), mul(lx, ly)}, minus_d, dbl(zkdev::to_mont(d)));
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
    const uint32_t* order;   // the key numbers sorted by those bytes (memcmp order); NULL where n == 1
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

// the host form: the statuses, the flags, and v of every search row into T->v
inline zk_status points_on_host(zk_elgamal_table* T, const Plan& pl, const Keys& keys, Found* f) {
    const size_t nm = pl.matches.size() - 1;
    std::vector<zkwit::JPoint> v(pl.n_search);
    WipeOnExit wipe_v{v.data(), v.size() * sizeof(zkwit::JPoint)};
    const unsigned nth = zkrt::host_threads(nm, 64);
    auto work = [&](unsigned th) {
        const size_t m0 = nm * th / nth, m1 = nm * (th + 1) / nth;
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
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        for (uint32_t r = r0; r < r1; r++) {
            const uint32_t out = pl.rows[r].out & ~ROW_ANON;
            v[out] = aff[r - r0];
            if (pl.rows[r].out & ROW_ANON) v[out + 1] = zkwit::JPoint{zkhost::Fr::zero() - aff[r - r0].x, aff[r - r0].y};
        }
    };
    zkrt::run_threads(nth, work);
    static_assert(sizeof(zkwit::JPoint) == 64, "x | y, the layout of zkdlog::Search::v");
    ZK_TRY(T->v.ensure(v.size() * 64));
    HIP_TRY(hipMemcpyAsync(T->v.p, v.data(), v.size() * 64, hipMemcpyHostToDevice, zkrt::g_stream));
    return ZK_OK;
}

// the device form: the same three, by two kernels.  head: the key-derived bytes the point kernel reads, at the start of scan_key
// (a multiple of 16; D follows them); launch_points starts that kernel.
template <class LaunchPoints>
inline zk_status points_on_device(zk_elgamal_table* T, const Plan& pl, const std::vector<uint8_t>& head, Found* f, LaunchPoints launch_points) {
    const size_t np = pl.points(), p64 = (np + 63) / 64 * 64, nm = pl.matches.size() - 1, nr = pl.rows.size();
    // scan_in: encodings (padded) | rights | rows.  scan_out: coordinates | statuses | flags.  scan_key: head | D
    std::vector<uint8_t> in(p64 * 32 + nm * 32 + nr * 16, 0);
    memcpy(in.data(), pl.enc.data(), np * 32);
    for (size_t m = 0; m < nm; m++) memcpy(&in[p64 * 32 + m * 32], &pl.enc[(size_t)pl.rows[pl.matches[m].row0].right_pt * 32], 32);
    static_assert(sizeof(Row) == 16, "four words");
    memcpy(&in[p64 * 32 + nm * 32], pl.rows.data(), nr * 16);
    const size_t key_bytes = head.size() + nm * 128;
    ZK_TRY(T->scan_in.ensure(in.size()));
    ZK_TRY(T->scan_out.ensure(np * 68 + nr * 4));
    ZK_TRY(T->scan_key.ensure(key_bytes));
    ZK_TRY(T->v.ensure((size_t)pl.n_search * 64));
    const uint32_t* d_enc = T->scan_in.as<uint32_t>();
    const uint32_t *d_right = d_enc + p64 * 8, *d_rows = d_right + nm * 8;
    uint32_t* d_xy = T->scan_out.as<uint32_t>();
    uint32_t *d_status = d_xy + np * 16, *d_flags = d_status + np;
    uint32_t* d_d = T->scan_key.as<uint32_t>() + head.size() / 4;
    auto run = [&]() -> zk_status {
        HIP_TRY(hipMemcpyAsync(T->scan_in.p, in.data(), in.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        HIP_TRY(hipMemcpyAsync(T->scan_key.p, head.data(), head.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        launch_points(dim3((unsigned)(p64 / 64 + (nm + 63) / 64)), d_enc, (uint32_t)np, (uint32_t)p64, d_right, (uint32_t)nm, T->scan_key.p, d_xy, d_status, d_d);
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps("scan_combine");
            ZK_LAUNCH(k_scan_combine, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_rows, (uint32_t)nr, (const uint32_t*)d_xy,
                      (const uint32_t*)d_status, (const uint32_t*)d_d, T->v.as<uint32_t>(), d_flags);
        }
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> back(np + nr);
        HIP_TRY(hipMemcpyAsync(back.data(), d_status, back.size() * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipMemsetAsync(T->scan_key.p, 0, key_bytes, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        for (size_t p = 0; p < np; p++) f->status[p] = (uint8_t)back[p];
        memcpy(f->flags.data(), &back[np], nr * 4);
        return ZK_OK;
    };
    const zk_status rc = run();
    if (rc != ZK_OK) {   // the head, D and v do not stay behind a failure either
        (void)hipMemsetAsync(T->scan_key.p, 0, key_bytes, zkrt::g_stream);
        (void)hipMemsetAsync(T->v.p, 0, (size_t)pl.n_search * 64, zkrt::g_stream);
        (void)hipStreamSynchronize(zkrt::g_stream);
    }
    return rc;
}
// one key: its width-4 NAF, recoded here once per call, and k_scan_points
inline zk_status points_one_key(zk_elgamal_table* T, const Plan& pl, const Keys& keys, Found* f) {
    std::vector<uint8_t> digits(DIGITS_BYTES);
    WipeOnExit wipe_digits{digits.data(), digits.size()};
    naf_recode(keys.scalar(0), digits.data());
    return points_on_device(T, pl, digits, f, [](dim3 grid, const uint32_t* enc, uint32_t np, uint32_t p64, const uint32_t* right, uint32_t nm, void* head,
                                                 uint32_t* xy, uint32_t* status, uint32_t* d) {
        zkrt::ProfScope ps("scan_points");
        ZK_LAUNCH(k_scan_points, grid, dim3(64), 0, zkrt::g_stream, enc, np, p64, right, nm, (const int8_t*)head, xy, status, d);
    });
}

// one slice: the point stage in the form the row count asks for, then the search over the rows resident in T->v
template <class Device>
inline zk_status decrypt_plan(zk_elgamal_table* T, Plan& pl, const Keys& keys, uint64_t limit, Found* f, Device device) {
    pl.close();
    f->status.assign(pl.points(), 0);
    f->flags.assign(pl.rows.size(), 0);
    f->x.assign(pl.n_search, ~0ull);
    if (pl.rows.empty()) return ZK_OK;
    ZK_TRY(pl.rows.size() <= host_max() ?points_on_host(T, pl, keys, f) : device(T, pl, keys, f));
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
//   device(T, plan, keys, found)     the device form of the point stage
//   slot(h, xt, key)                 where the result of match h - counted over the whole call, in (xt, key) order - goes; zeroed
template <class Kind, class Device, class Slot>
inline zk_status run(zk_elgamal_table* t, const Keys& keys, size_t n, const typename Kind::Xt* xts, uint64_t limit, Device device, Slot slot) {
    Plan pl;
    Found f;
    size_t done = 0;
    auto flush = [&]() -> zk_status {
        ZK_TRY(decrypt_plan(t, pl, keys, limit, &f, device));
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
    if (limit == 0 || limit > (1ull << 32)) return fail(ZK_ERR_INVALID_ARGUMENT, "limit must be 1 .. 2^32");
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
    return run<Kind>(t, Keys{1, dk, key, nullptr}, n, xts, limit, points_one_key, [out](size_t, size_t xt, uint32_t) { return &out[xt]; });
}

inline zk_status confidential(zk_elgamal_table* t, size_t n, const zk_confidential_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                              zk_confidential_scan_result* out) {
    return scan<Confidential>(t, n, xts, dec_key, limit, out);
}

inline zk_status anonymous(zk_elgamal_table* t, size_t n, const zk_anonymous_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                           zk_anonymous_scan_result* out) {
    return scan<Anonymous>(t, n, xts, dec_key, limit, out);
}

}  // namespace zkscan
