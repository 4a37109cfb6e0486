// The point stage behind the wallet's scans and its balance query (elgamal_scan.h, scan_keys.h, balance_keys.h): the entries match on
// the host, and every slice of their matches is brought to v = L - dk R, affine, in the table's v buffer, where the search of
// zk_elgamal_decrypt (witness.cpp elgamal_dlog_search_resident) finds the logarithms.  ONE stage, in two forms that leave the same bytes:
//   host    HostRows: the entry's own point work on the zk_set_host_threads pool (for_each_range), then one batch_to_affine per thread,
//           the scatter into v, one upload, and a synchronise before the host copy of v is wiped
//   device  device_stage: a Slice - encodings, right halves, key-derived head bytes, rows - through two launches on the library
//           stream, one wave per block, nothing in scratch memory:
//     the point kernel     point_lane, one lane per task, the two kinds split at a wave boundary (the point count is padded to 64)
//                            lanes [0, P)          read_point + is_prime_order: k_into_xy's body, the coordinates left in Montgomery form
//                            lanes [P64, P64 + R)  read_point of a right half, then D = [dk] right by the kernel's MULTIPLIER:
//       k_scan_points      NafMul: ONE key.  The width-4 NAF of dk, recoded on the host once per call: 252 doublings and an addition
//                          per non-zero digit against +-R, +-3R, +-5R, +-7R cached in LDS - is_prime_order's steps and its chain
//                          length (~3 000 dependent products with read_point's ~620).  Every lane reads the same digits, so a wave
//                          takes one path.  LDS as k_into_xy: [slot][word][lane], 16 slots, 32 768 B per block.
//       k_keys_points      BoothMul: the lane's OWN scalar.  A NAF would put every lane's additions at its own positions, so the
//                          chain is k_rj_check's: signed FIXED windows of W = 3 bits (booth_digit, read off the scalar's words in
//                          an LDS slot), three doublings per window and one ext_add_cached against 1 .. 4 times right where the
//                          digit is not zero - all 64 lanes add at the same 85 positions: 252 doublings (2 016 products), up to 85
//                          additions (680), the four cached multiples (~30), about 3 350 dependent products with read_point.
//                          LDS: slots 0 .. 15 the window table of read_point / is_prime_order, then the cached multiples
//                          (Y + X, Y - X, 2 d T, 2 Z); slot 16 the eight plain words of the lane's scalar (dynamic indexing of
//                          registers would go to scratch) = 17 x 32 x 64 = 34 816 B.
//     the combine kernel   one lane per row: k_scan_combine (elgamal_scan.h) or k_balance_combine (balance_keys.h)
// Secrets: the head (the digits of dk, or a scalar per right half), D, v and the logarithms are key-derived.  The head travels per
// call at the start of the table's scan_key buffer with D behind it, v in the table's v buffer; both are zeroed on the device after
// every call and on every failure, the host copies wiped on every way out.  The encodings, coordinates and statuses are public.
// The device form is NOT constant-time: the digits of dk decide where k_scan_points' shared chain adds, and k_keys_points skips the
// addition of a zero digit; the host forms multiply with jubjub_var_mul, whose steps do not depend on the scalar.
// Included by wallet.cpp below redjubjub.h (WipeOnExit, zkrj::ld_fr, zkrj::booth_digit), and by no other unit.
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
// (read per call; zk_balance_keys counts its hits against the same value)
inline size_t host_max() {
    const char* e = getenv("ZKAMD_SCAN_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
}
inline zk_status check_limit(uint64_t limit) {
    return limit == 0 || limit > (1ull << 32) ? fail(ZK_ERR_INVALID_ARGUMENT, "limit must be 1 .. 2^32") : ZK_OK;
}
constexpr uint32_t ROW_ANON = 1u << 31;   // with a search row: also store -v, one search row further
constexpr size_t DIGITS_BYTES = 272;      // 256 digits, their top index as an int32, padded to 16 bytes
constexpr int KEYS_WINDOW = 3, KEYS_MULTIPLES = 1 << (KEYS_WINDOW - 1);
constexpr uint32_t KEYS_SLOT_SCALAR = 16, KEYS_LDS_SLOTS = 17, KEYS_LDS_BYTES = KEYS_LDS_SLOTS * 32 * 64;
static_assert(252 % KEYS_WINDOW == 0, "the last window at bit 252 holds bit 251 alone");
static_assert(4 * KEYS_MULTIPLES <= (int)KEYS_SLOT_SCALAR && KEYS_LDS_BYTES <= 36864, "the cached multiples below the scalar, in k_rj_check's budget");

ZK_DI void st_fr(uint32_t* p, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// ---- the two multipliers: [scalar of right half r] (xm, ym), extended
struct NafMul {   // head: 256 signed digits, then their top index (int32) - the same for every lane
    const int8_t* digits;
    ZK_DI EP operator()(const Lds& L, uint32_t, const Fr& xm, const Fr& ym, const Fr& d2) const {
        return zkxt::mul_naf(L, xm, ym, d2, digits, *reinterpret_cast<const int32_t*>(digits + 256));
    }
};
struct BoothMul {   // head: 8 plain words per right half
    const uint32_t* scalars;
    ZK_DI EP operator()(const Lds& L, uint32_t r, const Fr& xm, const Fr& ym, const Fr& d2) const {
        L.st(KEYS_SLOT_SCALAR, zkrj::ld_fr(scalars + (size_t)r * 8));
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
        EP acc = zkxt::ep_neutral();
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
        return acc;
    }
};

// One lane of a point kernel.  enc: p64 x 8 words (n_points of them used).  xy: n_points x 16 words, x then y in Montgomery form,
// zero where refused.  status: n_points words, zkxt::INTO_XY_*.  enc_right: n_rights x 8 words.  d_out: n_rights x 32 words,
// X Y Z T of [scalar] right (the neutral element where the encoding is no point: its decode lane reports it).
template <class Mul>
ZK_DI void point_lane(const Lds& L, const uint32_t* enc, uint32_t n_points, uint32_t p64, const uint32_t* enc_right, uint32_t n_rights, const Mul& mul_right,
                      uint32_t* xy, uint32_t* status, uint32_t* d_out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
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
        EP acc = zkxt::ep_neutral();
        if (zkxt::read_point(L, enc_right + (size_t)r * 8, &x, &y, &xm, &ym, &d) == zkxt::INTO_XY_OK) acc = mul_right(L, r, xm, ym, dbl(d));
        uint32_t* o = d_out + (size_t)r * 32;
        st_fr(o, acc.X);
        st_fr(o + 8, acc.Y);
        st_fr(o + 16, acc.Z);
        st_fr(o + 24, acc.T);
    }
}
static __global__ void __launch_bounds__(64)
k_scan_points(const uint32_t* enc, uint32_t n_points, uint32_t p64, const uint32_t* enc_right, uint32_t n_rights, const int8_t* digits,
              uint32_t* xy, uint32_t* status, uint32_t* d_out) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    point_lane(Lds{table + threadIdx.x}, enc, n_points, p64, enc_right, n_rights, NafMul{digits}, xy, status, d_out);
}
static __global__ void __launch_bounds__(64)
k_keys_points(const uint32_t* enc, uint32_t n_points, uint32_t p64, const uint32_t* enc_right, uint32_t n_hits, const uint32_t* scalars,
              uint32_t* xy, uint32_t* status, uint32_t* d_out) {
    ZK_SHARED uint32_t table[KEYS_LDS_SLOTS * 8 * 64];
    point_lane(Lds{table + threadIdx.x}, enc, n_points, p64, enc_right, n_hits, BoothMul{scalars}, xy, status, d_out);
}

// ---- host side: the device form
// what a launch of the stage sees: the three regions of scan_in, the head and D in scan_key, the regions of scan_out, the table's v
struct StageBufs {
    const uint32_t *enc, *right, *rows;
    uint32_t np, p64, nm, n_rows;
    const void* head;
    uint32_t *d, *xy, *status, *out, *flags, *v;
    dim3 point_grid() const { return dim3(p64 / 64 + (nm + 63) / 64); }
    dim3 row_grid() const { return dim3((n_rows + 63) / 64); }
};
struct StageKernel {
    const char* name;   // of its ProfScope
    void (*launch)(const StageBufs&);   // (a named function: a launch inside a lambda of a namespace-scope initialiser starts nothing)
};
inline void launch_scan_points(const StageBufs& B) {
    ZK_LAUNCH(k_scan_points, B.point_grid(), dim3(64), 0, zkrt::g_stream, B.enc, B.np, B.p64, B.right, B.nm, (const int8_t*)B.head, B.xy, B.status, B.d);
}
inline void launch_keys_points(const StageBufs& B) {
    ZK_LAUNCH(k_keys_points, B.point_grid(), dim3(64), 0, zkrt::g_stream, B.enc, B.np, B.p64, B.right, B.nm, (const uint32_t*)B.head, B.xy, B.status, B.d);
}
const StageKernel SCAN_POINTS{"scan_points", launch_scan_points}, KEYS_POINTS{"keys_points", launch_keys_points};
// one slice of an entry's matches: at most ELGAMAL_SEARCH_BLOCK search rows
struct Slice {
    const std::vector<uint8_t>&enc, &rights, &head;   // 32 bytes per decode lane | per multiplication lane | the key-derived bytes (a multiple of 16)
    const void* rows;                                 // what the combine reads: n_rows x row_bytes
    size_t n_rows, row_bytes, out_bytes, n_search;    // out_bytes: per row, what the combine leaves to read back, its flag word last
    const StageKernel &points, &combine;
};
// The device form.  scan_in: encodings (padded to 64) | rights | rows.  scan_key: head | D.  scan_out: coordinates | the rows'
// output less their flags | flags | statuses.  out: n_rows x out_bytes as they lie there; status (or NULL): a byte per encoding.
// On any failure the head, D and the slice's rows of v are zeroed: the search, which wipes v on every way out, is not reached.
inline zk_status device_stage(zk_elgamal_table* T, const Slice& s, uint32_t* out, uint8_t* status) {
    const size_t np = s.enc.size() / 32, p64 = (np + 63) / 64 * 64, nm = s.rights.size() / 32, rows_at = (p64 + nm) * 32;
    const size_t key_bytes = s.head.size() + nm * 128, out_words = s.n_rows * s.out_bytes / 4;
    std::vector<uint8_t> in(rows_at + s.n_rows * s.row_bytes, 0);
    if (np) memcpy(in.data(), s.enc.data(), np * 32);
    if (nm) memcpy(&in[p64 * 32], s.rights.data(), nm * 32);
    memcpy(&in[rows_at], s.rows, s.n_rows * s.row_bytes);
    auto zero = [](zkrt::DevBuf& b, size_t n) { return n && b.cap >= n ? hipMemsetAsync(b.p, 0, n, zkrt::g_stream) : hipSuccess; };
    auto run = [&]() -> zk_status {
        ZK_TRY(T->scan_in.ensure(in.size()));
        ZK_TRY(T->scan_out.ensure(np * 68 + out_words * 4));
        ZK_TRY(T->scan_key.ensure(std::max<size_t>(key_bytes, 16)));
        ZK_TRY(T->v.ensure(s.n_search * 64));
        StageBufs B;
        B.enc = T->scan_in.as<uint32_t>(), B.right = B.enc + p64 * 8, B.rows = B.enc + rows_at / 4;
        B.np = (uint32_t)np, B.p64 = (uint32_t)p64, B.nm = (uint32_t)nm, B.n_rows = (uint32_t)s.n_rows;
        B.head = T->scan_key.p, B.d = T->scan_key.as<uint32_t>() + s.head.size() / 4;
        B.xy = T->scan_out.as<uint32_t>(), B.out = B.xy + np * 16, B.flags = B.out + out_words - s.n_rows, B.status = B.out + out_words;
        B.v = T->v.as<uint32_t>();
        HIP_TRY(hipMemcpyAsync(T->scan_in.p, in.data(), in.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        if (!s.head.empty()) HIP_TRY(hipMemcpyAsync(T->scan_key.p, s.head.data(), s.head.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        if (np) {   // (no lane: every encoding of the slice is the identity's)
            zkrt::ProfScope ps(s.points.name);
            s.points.launch(B);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps(s.combine.name);
            s.combine.launch(B);
        }
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> back(out_words + (status ? np : 0));
        HIP_TRY(hipMemcpyAsync(back.data(), B.out, back.size() * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(zero(T->scan_key, key_bytes));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(out, back.data(), out_words * 4);
        for (size_t p = 0; status && p < np; p++) status[p] = (uint8_t)back[out_words + p];
        return ZK_OK;
    };
    const zk_status rc = run();
    if (rc != ZK_OK) {
        (void)zero(T->scan_key, key_bytes);
        (void)zero(T->v, s.n_search * 64);
        (void)hipStreamSynchronize(zkrt::g_stream);
    }
    return rc;
}

// ---- host side: where both host forms end.  v: one affine point per search row of the slice, wiped on the way out.
struct HostRows {
    std::vector<zkwit::JPoint> v;
    explicit HostRows(size_t n_search) : v(n_search) {}
    ~HostRows() {
        if (!v.empty()) explicit_bzero(v.data(), v.size() * sizeof(zkwit::JPoint));
    }
    // a thread's share: its projective points to affine form by one inversion; every stride-th of them from `first` is a row's v and
    // goes to the search row out(k) names - with ROW_ANON also as -v, one search row further
    template <class Out>
    void land(const std::vector<zkwit::EPoint>& proj, std::vector<zkwit::JPoint>& aff, size_t first, size_t stride, Out out) {
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        for (size_t k = 0; first + k * stride < aff.size(); k++) {
            const zkwit::JPoint& a = aff[first + k * stride];
            const uint32_t o = out(k);
            v[o & ~ROW_ANON] = a;
            if (o & ROW_ANON) v[(o & ~ROW_ANON) + 1] = zkwit::JPoint{zkhost::Fr::zero() - a.x, a.y};
        }
    }
    // after the threads: v into T->v, and done before this object goes (an asynchronous copy would read v while it is wiped and freed)
    zk_status upload(zk_elgamal_table* T) {
        static_assert(sizeof(zkwit::JPoint) == 64, "x | y, the layout of zkdlog::Search::v");
        auto run = [&]() -> zk_status {
            ZK_TRY(T->v.ensure(v.size() * 64));
            HIP_TRY(hipMemcpyAsync(T->v.p, v.data(), v.size() * 64, hipMemcpyHostToDevice, zkrt::g_stream));
            HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
            return ZK_OK;
        };
        const zk_status rc = run();
        if (rc != ZK_OK && T->v.cap >= v.size() * 64) {   // as device_stage: v does not stay behind a failure
            (void)hipMemsetAsync(T->v.p, 0, v.size() * 64, zkrt::g_stream);
            (void)hipStreamSynchronize(zkrt::g_stream);
        }
        return rc;
    }
};

}  // namespace zkscan
