// The balances of the accounts of a key SET in one call (zk_balance_keys): BalanceQuery::get_balance_from_decryption_key
// (zface/src/utils/getter.rs:135-175) - EncryptedBalance + PendingTransfer by Ciphertext::add (elgamal.rs:139-148), the 64 bytes of
// the total by Ciphertext::write, and Ciphertext::decrypt of it (elgamal.rs:85-108) - for every account whose enc_key is a key of
// the set.  The accounts are the zk_block_account of the block executors; an account that carries ZK_BLOCK_ROLLOVER_DUE is read as
// balance + pending, any other as balance alone (its pending is not looked at).
// Included by wallet.cpp below scan_keys.h (zkscan::Keys, with_hits, read_prime_order), and by no other unit.
//
// The host matches the enc_key of every account against the key set's index - a hit is one account - and brings every hit to
//   L = lb (+ lp), R = rb (+ rp), v = L - dk R     (dk the scalar of the hit's key)
// L and R affine and written as Point::write does, v through the point stage (wallet_stage.h).  Its two forms here, the same bytes:
//   host    per hit read_prime_order of the two or four used points, ext_add of the halves, ONE jubjub_var_mul of the summed right
//           half, v = L - D; HostRows over L, R and v
//   device  k_keys_points as it is.  Point lanes: the used encodings of all hits.  Multiplication lanes: one per used right half,
//           with the scalar of its hit - dk (rb + rp) = dk rb + dk rp, so a due account takes two lanes side by side, not a chain
//           twice as long.  Then
//     k_balance_combine  one lane per hit.  From a row of indices it takes the hit's decoded points and its one or two D and forms
//                        L, R and V = L - Db - Dp by four ext_add (an absent operand is the neutral element: the law is complete
//                        on the prime-order subgroup, the identity included), inverts Z_L Z_R Z_V once (Montgomery's trick, pow_windows
//                        over digits_inverse(): ~330) and stores V's x, y in Montgomery form straight into the table's v buffer at the
//                        hit's search row, Point::write of L and R (zkxt::point_write, as k_ledger_encode) and one flag word: 0, or
//                        field | status << 6 of the first refused used point.  A refused hit stores the neutral element and zero
//                        bytes.  About 36 + 330 + 12: ~400 dependent products.
//                        LDS: pow_windows' table, [slot][word][lane], 16 x 32 x 64 = 32 768 B; nothing in scratch memory.
//   An encoding whose 32 bytes are the identity's (the empty pending transfer, Ciphertext::zero()) gets no lane in the device form:
//   the combine takes the neutral element for it, which is what decoding it gives.
// Secrets: as wallet_stage.h, and the values.  The encodings, statuses and enc_total are public chain data.
#pragma once
#include "scan_keys.h"

namespace zkscan {

constexpr uint32_t BAL_NONE = 0xffffffffu;   // in a row: no lane - the neutral element (an unused or an identity encoding)
enum { F_BALANCE_LEFT = 1, F_BALANCE_RIGHT = 2, F_PENDING_LEFT = 3, F_PENDING_RIGHT = 4 };

ZK_DI EP bal_point(const uint32_t* xy, uint32_t p) {
    if (p == BAL_NONE) return zkxt::ep_neutral();
    const Fr x = zkrj::ld_fr(xy + (size_t)p * 16), y = zkrj::ld_fr(xy + (size_t)p * 16 + 8);
    return EP{x, y, Fr::one(), mul(x, y)};
}
ZK_DI EP bal_minus_d(const uint32_t* d_in, uint32_t r) {
    if (r == BAL_NONE) return zkxt::ep_neutral();
    const uint32_t* dd = d_in + (size_t)r * 32;
    return EP{neg(zkrj::ld_fr(dd)), zkrj::ld_fr(dd + 8), zkrj::ld_fr(dd + 16), neg(zkrj::ld_fr(dd + 24))};
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
        const Fr d2 = zkxt::jubjub_d2();
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
        zkxt::point_write(o, mul(sl.X, zl), mul(sl.Y, zl));
        zkxt::point_write(o + 8, mul(sr.X, zr), mul(sr.Y, zr));
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

inline void launch_balance_combine(const StageBufs& B) {
    ZK_LAUNCH(k_balance_combine, B.row_grid(), dim3(64), 0, zkrt::g_stream, B.rows, B.n_rows, (const uint32_t*)B.xy, (const uint32_t*)B.status,
              (const uint32_t*)B.d, B.v, B.out, B.flags);
}
const StageKernel BALANCE_COMBINE{"balance_combine", launch_balance_combine};

// the host form: the refusals, the bytes, and v of every hit into T->v
inline zk_status balance_on_host(zk_elgamal_table* T, const Keys& keys, const zk_block_account* accounts, const BalanceHit* hits, size_t nh, BalanceFound* f) {
    HostRows hr(nh);
    ZK_TRY(zkrt::for_each_range(nh, 64, [&](size_t h0, size_t h1) -> zk_status {
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
        hr.land(proj, aff, 2, 3, [&](size_t k) { return (uint32_t)(h0 + k); });
        for (size_t h = h0; h < h1; h++) {
            const zkwit::JPoint* p = &aff[3 * (h - h0)];
            if (f->refusal[h]) continue;
            jubjub_encode(p[0].x, p[0].y, &f->enc[h * 64]);
            jubjub_encode(p[1].x, p[1].y, &f->enc[h * 64 + 32]);
        }
        return ZK_OK;
    }));
    return hr.upload(T);
}

// the device form: the same three, by k_keys_points and k_balance_combine
inline zk_status balance_on_device(zk_elgamal_table* T, const Keys& keys, const zk_block_account* accounts, const BalanceHit* hits, size_t nh, BalanceFound* f) {
    static const uint8_t identity[32] = {1};
    std::vector<uint8_t> enc, rights, scalars;
    std::vector<uint32_t> rows(nh * 8, 0), out(nh * 17);
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
    ZK_TRY(device_stage(T, Slice{enc, rights, scalars, rows.data(), nh, 32, 68, nh, KEYS_POINTS, BALANCE_COMBINE}, out.data(), nullptr));
    memcpy(f->enc.data(), out.data(), nh * 64);
    for (size_t h = 0; h < nh; h++) f->refusal[h] = (uint8_t)out[nh * 16 + h];
    return ZK_OK;
}

// hits_out[h]: the h-th account, in account order, whose enc_key is a key of the set.  Matching runs first, before any other work.
inline zk_status balance_keys(zk_elgamal_table* t, const zk_scan_keys* k, size_t n, const zk_block_account* accounts, uint64_t limit,
                              zk_balance_hit* hits_out, size_t hits_cap, size_t* n_hits_out) {
    std::vector<BalanceHit> hits;
    return with_hits(
        t, k, n, accounts, limit, "a hit numbers its account in 32 bits: n_accounts must be below 2^32", "these accounts", hits_out, hits_cap, n_hits_out,
        [&](const Keys& keys) -> size_t {
            for (size_t i = 0; i < n; i++) {
                const int64_t key = keys.find(accounts[i].enc_key);
                if (key >= 0) hits.push_back(BalanceHit{(uint32_t)i, (uint32_t)key, (accounts[i].flags & ZK_BLOCK_ROLLOVER_DUE) != 0});
            }
            return hits.size();
        },
        [&](const Keys& keys, size_t total) -> zk_status {
            const size_t host_hits = host_max();
            for (size_t first = 0; first < total; first += ELGAMAL_SEARCH_BLOCK) {   // slices of at most one search launch
                const size_t nh = std::min(ELGAMAL_SEARCH_BLOCK, total - first);
                BalanceFound f;
                f.refusal.assign(nh, 0);
                f.enc.assign(nh * 64, 0);
                std::vector<uint64_t> x(nh, ~0ull);
                WipeOnExit wipe_x{x.data(), x.size() * sizeof(uint64_t)};
                ZK_TRY((nh <= host_hits ? balance_on_host : balance_on_device)(t, keys, accounts, &hits[first], nh, &f));
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
        });
}

}  // namespace zkscan
