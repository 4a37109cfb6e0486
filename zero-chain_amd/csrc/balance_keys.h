// The balances of the accounts of a key SET in one call (zk_balance_keys): BalanceQuery::get_balance_from_decryption_key
// (zface/src/utils/getter.rs:135-175) - EncryptedBalance + PendingTransfer by Ciphertext::add (elgamal.rs:139-148), the 64 bytes of
// the total by Ciphertext::write, and Ciphertext::decrypt of it (elgamal.rs:85-108) - for every account whose enc_key is a key of
// the set.  The accounts are the zk_block_account of the block executors; an account that carries ZK_BLOCK_ROLLOVER_DUE is read as
// balance + pending, any other as balance alone (its pending is not looked at).
// Included by wallet.cpp below scan_keys.h (zkscan::Keys, k_keys_points, host_max, read_prime_order, st_fr), and by no other unit.
//
// The host matches the enc_key of every account against the key set's index - a hit is one account - and brings every hit to
//   L = lb (+ lp), R = rb (+ rp), v = L - dk R     (dk the scalar of the hit's key)
// L and R affine and written as Point::write does, v affine in the table's v buffer, where the search of zk_elgamal_decrypt
// (witness.cpp elgamal_dlog_search_resident) finds the logarithm.  Two forms of the point work, the same bytes:
//   host    per hit read_prime_order of the two or four used points, ext_add of the halves, ONE jubjub_var_mul of the summed right
//           half, v = L - D; one batch_to_affine per thread over L, R and v; one upload of v
//   device  two launches on the library stream, one wave per block:
//     k_keys_points      as it is (scan_keys.h).  Point lanes: the used encodings of all hits, read_point + is_prime_order each.
//                        Multiplication lanes: one per used right half, with the scalar of its hit - dk (rb + rp) = dk rb + dk rp,
//                        so a due account takes two lanes side by side, not a chain twice as long: ~3 350 dependent products.
//     k_balance_combine  one lane per hit.  From a row of indices it takes the hit's decoded points and its one or two D and forms
//                        L, R and V = L - Db - Dp by four ext_add (an absent operand is the neutral element: the law is complete
//                        on the prime-order subgroup, the identity included), inverts Z_L Z_R Z_V once (Montgomery's trick, pow_windows
//                        over digits_inverse(): ~330) and stores V's x, y in Montgomery form straight into the table's v buffer at the
//                        hit's search row, Point::write of L and R (from_mont, the parity of x into the top bit, as k_ledger_encode)
//                        and one flag word: 0, or field | status << 6 of the first refused used point.  A refused hit stores the
//                        neutral element and zero bytes.  About 36 + 330 + 12: ~400 dependent products.
//                        LDS: pow_windows' table, [slot][word][lane], 16 x 32 x 64 = 32 768 B; nothing in scratch memory.
//   An encoding whose 32 bytes are the identity's (the empty pending transfer, Ciphertext::zero()) gets no lane in the device form:
//   the combine takes the neutral element for it, which is what decoding it gives.
// Secrets: the per-hit scalars, D, v, the logarithms and the values are key-derived.  The scalars travel per call in the head of the
// table's scan_key buffer with D behind them, v in the table's v buffer; both are zeroed on the device after every call and on every
// failure path, the host copies wiped on every way out.  The encodings, statuses and enc_total are public chain data.
// The device form is NOT constant-time: k_keys_points skips the addition of a zero digit, so a lane's path depends on its scalar;
// the host form multiplies with jubjub_var_mul, whose steps do not depend on it.
#pragma once
#include "scan_keys.h"

namespace zkscan {

constexpr uint32_t BAL_NONE = 0xffffffffu;   // in a row: no lane - the neutral element (an unused or an identity encoding)
enum { F_BALANCE_LEFT = 1, F_BALANCE_RIGHT = 2, F_PENDING_LEFT = 3, F_PENDING_RIGHT = 4 };

ZK_DI EP bal_point(const uint32_t* xy, uint32_t p) {
    if (p == BAL_NONE) return EP{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
    const Fr x = zkrj::ld_fr(xy + (size_t)p * 16), y = zkrj::ld_fr(xy + (size_t)p * 16 + 8);
    return EP{x, y, Fr::one(), mul(x, y)};
}
ZK_DI EP bal_minus_d(const uint32_t* d_in, uint32_t r) {
    if (r == BAL_NONE) return EP{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
    const uint32_t* dd = d_in + (size_t)r * 32;
    return EP{neg(zkrj::ld_fr(dd)), zkrj::ld_fr(dd + 8), zkrj::ld_fr(dd + 16), neg(zkrj::ld_fr(dd + 24))};
}
ZK_DI void bal_write(uint32_t* o, const Fr& x_mont, const Fr& y_mont) {   // edwards::Point::write
    const Fr x = zkdev::from_mont(x_mont);
    Fr y = zkdev::from_mont(y_mont);
    y.l[7] |= (x.l[0] & 1u) << 31;
    st_fr(o, y);
}

// rows: n_hits x 8 words - the points balance left, balance right, pending left, pending right; the multiplication lanes of the two
// right halves; the search row; 0.  BAL_NONE where there is none.  xy, status: k_keys_points' of the points, d_in its d_out.
// v: the table's buffer (zkdlog::Search::v: per search row x then y, Montgomery).  enc: n_hits x 16 words, left | right.  flags: n_hits words.
static __global__ void __launch_bounds__(64)
k_balance_combine(const uint32_t* rows, uint32_t n_hits, const uint32_t* xy, const uint32_t* status, const uint32_t* d_in, uint32_t* v,
                  uint32_t* enc, uint32_t* flags) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_hits) return;
    const Lds lds{table + threadIdx.x};
    const uint4 pts = reinterpret_cast<const uint4*>(rows)[2 * (size_t)i], rest = reinterpret_cast<const uint4*>(rows)[2 * (size_t)i + 1];
    uint32_t refusal = 0;   // the first in the order of the fields: the last one written here
    if (pts.w != BAL_NONE && status[pts.w]) refusal = F_PENDING_RIGHT | status[pts.w] << 6;
    if (pts.z != BAL_NONE && status[pts.z]) refusal = F_PENDING_LEFT | status[pts.z] << 6;
    if (pts.y != BAL_NONE && status[pts.y]) refusal = F_BALANCE_RIGHT | status[pts.y] << 6;
    if (pts.x != BAL_NONE && status[pts.x]) refusal = F_BALANCE_LEFT | status[pts.x] << 6;
    Fr vx = Fr::zero(), vy = Fr::one();
    uint32_t* o = enc + (size_t)i * 16;
    if (!refusal) {
        Fr d2;
        {
            const uint64_t dp[4] = ZK_JUBJUB_D_PLAIN_64;
#pragma unroll
            for (int k = 0; k < 8; k++) d2.l[k] = (uint32_t)(dp[k >> 1] >> (32 * (k & 1)));
            d2 = dbl(zkdev::to_mont(d2));
        }
        const EP sl = zkxt::ext_add(bal_point(xy, pts.x), bal_point(xy, pts.z), d2);
        const EP sr = zkxt::ext_add(bal_point(xy, pts.y), bal_point(xy, pts.w), d2);
        const EP sv = zkxt::ext_add(sl, zkxt::ext_add(bal_minus_d(d_in, rest.x), bal_minus_d(d_in, rest.y), d2), d2);
        // 1 / Z of all three from one inversion (no Z is zero: the addition law is complete on the prime-order subgroup)
        const Fr lr = mul(sl.Z, sr.Z);
        constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
        const Fr inv = zkxt::pow_windows(lds, mul(lr, sv.Z), EI);
        const Fr zv = mul(inv, lr), t = mul(inv, sv.Z);
        const Fr zl = mul(t, sr.Z), zr = mul(t, sl.Z);
        vx = mul(sv.X, zv);
        vy = mul(sv.Y, zv);
        bal_write(o, mul(sl.X, zl), mul(sl.Y, zl));
        bal_write(o + 8, mul(sr.X, zr), mul(sr.Y, zr));
    } else {
        st_fr(o, Fr::zero());
        st_fr(o + 8, Fr::zero());
    }
    st_fr(v + (size_t)rest.z * 16, vx);
    st_fr(v + (size_t)rest.z * 16 + 8, vy);
    flags[i] = refusal;
}

// ---- host side
struct BalanceHit {
    uint32_t account, key;
    bool due;   // ZK_BLOCK_ROLLOVER_DUE: pending is used
};
// what the point stage leaves of one slice: per hit the refusal byte and Ciphertext::write of the total (zero bytes where refused)
struct BalanceFound {
    std::vector<uint8_t> refusal, enc;
};
// the encoding of field f (F_*) of an account
inline const uint8_t* balance_field(const zk_block_account& a, int f) { return (f <= F_BALANCE_RIGHT ? a.balance : a.pending) + 32 * ((f - 1) & 1); }

// the host form: the refusals, the bytes, and v of every hit into T->v
inline zk_status balance_on_host(zk_elgamal_table* T, const Keys& keys, const zk_block_account* accounts, const BalanceHit* hits, size_t nh, BalanceFound* f) {
    std::vector<zkwit::JPoint> v(nh);
    WipeOnExit wipe_v{v.data(), v.size() * sizeof(zkwit::JPoint)};
    const unsigned nth = zkrt::host_threads(nh, 64);
    auto work = [&](unsigned th) {
        const size_t h0 = nh * th / nth, h1 = nh * (th + 1) / nth;
        std::vector<zkwit::EPoint> proj(3 * (h1 - h0), zkwit::ext_zero());   // L, R, v of every hit; a refused hit's stay neutral
        std::vector<zkwit::JPoint> aff(proj.size());
        WipeOnExit wipe_p{proj.data(), proj.size() * sizeof(zkwit::EPoint)}, wipe_a{aff.data(), aff.size() * sizeof(zkwit::JPoint)};
        for (size_t h = h0; h < h1; h++) {
            const zk_block_account& a = accounts[hits[h].account];
            zkwit::JPoint pt[4];
            const int used = hits[h].due ? 4 : 2;
            for (int k = 0; k < used && !f->refusal[h]; k++) {
                const uint8_t st = read_prime_order(balance_field(a, k + 1), &pt[k]);
                if (st) f->refusal[h] = (uint8_t)((k + 1) | st << 6);
            }
            if (f->refusal[h]) continue;
            zkwit::EPoint l = zkwit::to_ext(pt[0]), r = zkwit::to_ext(pt[1]);
            if (hits[h].due) {
                l = zkwit::ext_add(l, zkwit::to_ext(pt[2]));
                r = zkwit::ext_add(r, zkwit::to_ext(pt[3]));
            }
            const zkwit::EPoint s = jubjub_var_mul(r, keys.scalar(hits[h].key));
            zkwit::EPoint* p = &proj[3 * (h - h0)];
            p[0] = l;
            p[1] = r;
            p[2] = zkwit::ext_add(l, zkwit::EPoint{zkhost::Fr::zero() - s.X, s.Y, s.Z, zkhost::Fr::zero() - s.T});
        }
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        for (size_t h = h0; h < h1; h++) {
            const zkwit::JPoint* p = &aff[3 * (h - h0)];
            v[h] = p[2];
            if (f->refusal[h]) continue;
            jubjub_encode(p[0].x, p[0].y, &f->enc[h * 64]);
            jubjub_encode(p[1].x, p[1].y, &f->enc[h * 64 + 32]);
        }
    };
    zkrt::run_threads(nth, work);
    static_assert(sizeof(zkwit::JPoint) == 64, "x | y, the layout of zkdlog::Search::v");
    ZK_TRY(T->v.ensure(v.size() * 64));
    HIP_TRY(hipMemcpyAsync(T->v.p, v.data(), v.size() * 64, hipMemcpyHostToDevice, zkrt::g_stream));
    HIP_TRY(hipStreamSynchronize(zkrt::g_stream));   // (v is wiped when this returns)
    return ZK_OK;
}

// the device form: the same three, by k_keys_points and k_balance_combine
inline zk_status balance_on_device(zk_elgamal_table* T, const Keys& keys, const zk_block_account* accounts, const BalanceHit* hits, size_t nh, BalanceFound* f) {
    static const uint8_t identity[32] = {1};
    std::vector<uint8_t> enc, rights, scalars;
    std::vector<uint32_t> rows(nh * 8, 0);
    scalars.reserve(nh * 64);   // (two right halves per hit at the most: the vector never moves, and what is wiped below is all of it)
    WipeOnExit wipe_scalars{scalars.data(), nh * 64};
    for (size_t h = 0; h < nh; h++) {
        const zk_block_account& a = accounts[hits[h].account];
        uint32_t* row = &rows[h * 8];
        for (int k = 0; k < 6; k++) row[k] = BAL_NONE;
        for (int k = 0; k < (hits[h].due ? 4 : 2); k++) {
            const uint8_t* e = balance_field(a, k + 1);
            if (!memcmp(e, identity, 32)) continue;   // the neutral element needs no lane
            row[k] = (uint32_t)(enc.size() / 32);
            enc.insert(enc.end(), e, e + 32);
            if (k & 1) {   // a right half: its multiplication lane, with the scalar of the hit
                row[4 + (k >> 1)] = (uint32_t)(rights.size() / 32);
                rights.insert(rights.end(), e, e + 32);
                const uint8_t* s = reinterpret_cast<const uint8_t*>(keys.scalar(hits[h].key));
                scalars.insert(scalars.end(), s, s + 32);
            }
        }
        row[6] = (uint32_t)h;
    }
    const size_t np = enc.size() / 32, p64 = (np + 63) / 64 * 64, nm = rights.size() / 32;
    // scan_in: encodings (padded) | rights | rows.  scan_out: coordinates | bytes of the totals | flags | statuses.  scan_key: scalars | D
    std::vector<uint8_t> in(p64 * 32 + nm * 32 + nh * 32, 0);
    if (np) memcpy(in.data(), enc.data(), np * 32);
    if (nm) memcpy(&in[p64 * 32], rights.data(), nm * 32);
    memcpy(&in[p64 * 32 + nm * 32], rows.data(), nh * 32);
    const size_t key_bytes = nm * 32 + nm * 128;
    ZK_TRY(T->scan_in.ensure(in.size()));
    ZK_TRY(T->scan_out.ensure(np * 64 + nh * 64 + nh * 4 + np * 4));
    ZK_TRY(T->scan_key.ensure(std::max<size_t>(key_bytes, 16)));
    ZK_TRY(T->v.ensure(nh * 64));
    const uint32_t* d_enc = T->scan_in.as<uint32_t>();
    const uint32_t *d_right = d_enc + p64 * 8, *d_rows = d_right + nm * 8;
    uint32_t* d_xy = T->scan_out.as<uint32_t>();
    uint32_t *d_total = d_xy + np * 16, *d_flags = d_total + nh * 16, *d_status = d_flags + nh;
    uint32_t* d_d = T->scan_key.as<uint32_t>() + nm * 8;
    auto run = [&]() -> zk_status {
        HIP_TRY(hipMemcpyAsync(T->scan_in.p, in.data(), in.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        if (nm) HIP_TRY(hipMemcpyAsync(T->scan_key.p, scalars.data(), scalars.size(), hipMemcpyHostToDevice, zkrt::g_stream));
        if (np) {
            zkrt::ProfScope ps("keys_points");
            ZK_LAUNCH(k_keys_points, dim3((unsigned)(p64 / 64 + (nm + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_enc, (uint32_t)np, (uint32_t)p64, d_right,
                      (uint32_t)nm, (const uint32_t*)T->scan_key.p, d_xy, d_status, d_d);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps("balance_combine");
            ZK_LAUNCH(k_balance_combine, dim3((unsigned)((nh + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_rows, (uint32_t)nh, (const uint32_t*)d_xy,
                      (const uint32_t*)d_status, (const uint32_t*)d_d, T->v.as<uint32_t>(), d_total, d_flags);
        }
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> back(nh * 17);
        HIP_TRY(hipMemcpyAsync(back.data(), d_total, back.size() * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        if (key_bytes) HIP_TRY(hipMemsetAsync(T->scan_key.p, 0, key_bytes, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(f->enc.data(), back.data(), nh * 64);
        for (size_t h = 0; h < nh; h++) f->refusal[h] = (uint8_t)back[nh * 16 + h];
        return ZK_OK;
    };
    const zk_status rc = run();
    if (rc != ZK_OK && key_bytes) {   // the scalars and D do not stay behind a failure either (v: the caller's wipe)
        (void)hipMemsetAsync(T->scan_key.p, 0, key_bytes, zkrt::g_stream);
        (void)hipStreamSynchronize(zkrt::g_stream);
    }
    return rc;
}

// hits_out[h]: the h-th account, in account order, whose enc_key is a key of the set.  Matching runs first, before any other work.
inline zk_status balance_keys(zk_elgamal_table* t, const zk_scan_keys* k, size_t n, const zk_block_account* accounts, uint64_t limit,
                              zk_balance_hit* hits_out, size_t hits_cap, size_t* n_hits_out) {
    if (!t || !k || !n_hits_out || (n && !accounts)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (limit == 0 || limit > (1ull << 32)) return fail(ZK_ERR_INVALID_ARGUMENT, "limit must be 1 .. 2^32");
    *n_hits_out = 0;
    if (n == 0) return ZK_OK;
    if (n > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, "a hit numbers its account in 32 bits: n_accounts must be below 2^32");
    const Keys keys{k->n(), k->dk.data(), k->enc.data(), k->order.data()};
    std::vector<BalanceHit> hits;
    for (size_t i = 0; i < n; i++) {
        const int64_t key = keys.find(accounts[i].enc_key);
        if (key >= 0) hits.push_back(BalanceHit{(uint32_t)i, (uint32_t)key, (accounts[i].flags & ZK_BLOCK_ROLLOVER_DUE) != 0});
    }
    const size_t total = hits.size();
    if (total > hits_cap) {
        *n_hits_out = total;
        return fail(ZK_ERR_INVALID_ARGUMENT, "hits_cap " + std::to_string(hits_cap) + " is below the " + std::to_string(total) + " hits of these accounts");
    }
    if (total == 0) return ZK_OK;
    if (!hits_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(zkrt::use_device(t->device));
    memset(hits_out, 0, total * sizeof(zk_balance_hit));
    const size_t host_hits = host_max();
    auto run = [&]() -> zk_status {
        for (size_t first = 0; first < total; first += ELGAMAL_SEARCH_BLOCK) {   // slices of at most one search launch
            const size_t nh = std::min(ELGAMAL_SEARCH_BLOCK, total - first);
            BalanceFound f;
            f.refusal.assign(nh, 0);
            f.enc.assign(nh * 64, 0);
            std::vector<uint64_t> x(nh, ~0ull);
            WipeOnExit wipe_x{x.data(), x.size() * sizeof(uint64_t)};
            const zk_status stage = (nh <= host_hits ? balance_on_host : balance_on_device)(t, keys, accounts, &hits[first], nh, &f);
            if (stage != ZK_OK) {   // v may be on the device already; the search, which wipes it on every way out, is not reached
                if (t->v.cap >= nh * 64) (void)hipMemsetAsync(t->v.p, 0, nh * 64, zkrt::g_stream);
                (void)hipStreamSynchronize(zkrt::g_stream);
                return stage;
            }
            ZK_TRY(elgamal_dlog_search_resident(t, nh, limit, x.data()));
            for (size_t h = 0; h < nh; h++) {
                zk_balance_hit& o = hits_out[first + h];
                o.account = hits[first + h].account;
                o.key = hits[first + h].key;
                o.r.pending_added = hits[first + h].due ? 1 : 0;
                if ((o.r.refusal = f.refusal[h]) != 0) continue;
                memcpy(o.r.enc_total, &f.enc[h * 64], 64);
                if (x[h] < limit) {   // (the search reports ~0 for none)
                    o.r.found = 1;
                    o.r.value = (uint32_t)x[h];
                }
            }
        }
        return ZK_OK;
    };
    const zk_status rc = run();
    if (rc != ZK_OK) {   // a half-written array does not leave the call
        explicit_bzero(hits_out, total * sizeof(zk_balance_hit));
        return rc;
    }
    *n_hits_out = total;
    return ZK_OK;
}

}  // namespace zkscan
