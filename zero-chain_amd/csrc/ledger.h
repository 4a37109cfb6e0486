// A block's ElGamal balance updates: Ciphertext::add / Ciphertext::sub applied in order to stored ciphertexts, as the three
// balance modules of the reference do around every proof (zk_elgamal_ledger_apply):
//   modules/encrypted-balances/src/lib.rs:133-222, modules/encrypted-assets/src/lib.rs:266-350 (rollover, sub_enc_balance,
//   add_pending_transfer), modules/anonymous-balances/src/lib.rs:169-225 (twelve updates per extrinsic); the arithmetic is
//   core/primitives/src/ciphertext.rs:90-100 over elgamal::Ciphertext::read (both points through Point::read, as_prime_order).
// n_slots stored ciphertexts, n_ops updates in index order, each on one slot.  The result of a slot is its value plus the
// signed sum of its ops; the value an op meets (before_out) is the slot's plus the sum of the ops of that slot before it: a
// SEGMENTED EXCLUSIVE SCAN of Jubjub points over the ops in slot-major order.
//
// Two forms, the same bytes (Point::write of an affine point is canonical, so the order of summation does not show):
//   host    into_xy_one for every point on the zk_set_host_threads pool, a stable counting sort of the ops by slot, each
//           slot's ops walked in extended coordinates, one batch_to_affine per thread's share
//   device  1. k_into_xy (xt_inputs.h) over all 2 (n_slots + n_ops) encodings in one launch, nothing copied back  ~3 200 / point
//           2. the host groups the ops by slot meanwhile (offsets, a permutation and its inverse)
//           3. k_ledger_scan: one lane per op and component (left: blockIdx.y = 0, right: 1), LEDGER_SCAN_W lanes per
//              workgroup.  A lane forms its addend (2 products to Montgomery form, 1 for T; X and T negated for a subtraction;
//              the identity where the op is refused or skipped), then log2 W = 8 Kogge-Stone steps of ext_add (9 products) in
//              LDS.  No head flags travel: a lane knows how many lanes to its left belong to its slot (its index minus the
//              slot's first op, from the offsets) and takes lane t - d exactly when d is no more than that.  It writes the
//              exclusive prefix of every op, the sum of every slot that ENDS in the workgroup and the workgroup's tail.  ~75
//              k_ledger_carry: the same scan over the workgroups' tails, W at a time with a running carry, for a slot with more
//              ops than one workgroup or one that straddles a boundary (the host names, per workgroup, the last one at or
//              before it in which a slot starts).                                                                       ~75
//           4. k_ledger_encode: one lane per output point (2 n_slots, and 2 n_ops more with before_out): the slot's value +
//              carry + prefix (the fix-up is the carry's addition here: at most two ext_add), 1 / Z by pow_windows over
//              digits_inverse(), from_mont, the parity of x into the top bit; zero bytes where the slot was refused.      ~360
//           5. one copy back: the statuses of all points and the encodings
//           LDS: the scan keeps one EP per lane, [X Y Z T][word][lane] - 4 x 8 x 256 words = 32 KB, every lane in its own
//           bank; the encoder keeps pow_windows' table, 16 x 8 x 64 words = 32 KB.  Nothing in scratch memory.
// A slot that holds every op of the call is W lanes wide like any other: no lane walks a slot.
// Only verify.cpp includes this header (it needs xt_inputs.h, and the library carries ONE k_into_xy).
// The data is public chain state: nothing here is constant-time, and the buffers are freed without the wipe.
#pragma once
#include "xt_inputs.h"

namespace zkledger {

using zkdev::Fr;
using zkrt::fail;
using zkxt::EP;

constexpr uint32_t LEDGER_SCAN_W = 256;   // lanes of a workgroup of the scan (zero_chain_amd.LEDGER_SCAN_WIDTH restates it)
constexpr uint32_t LEDGER_SUB = 1, LEDGER_SKIP = 2;

// ---- device side
ZK_DI Fr fr_load(const uint32_t* g) {
    const uint4* q = reinterpret_cast<const uint4*>(g);
    const uint4 lo = q[0], hi = q[1];
    Fr r;
    r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
    r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
    return r;
}
ZK_DI void fr_store(uint32_t* g, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(g);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
// an EP in global memory: 32 words, X Y Z T
ZK_DI EP ep_load(const uint32_t* g) { return EP{fr_load(g), fr_load(g + 8), fr_load(g + 16), fr_load(g + 24)}; }
ZK_DI void ep_store(uint32_t* g, const EP& p) {
    fr_store(g, p.X);
    fr_store(g + 8, p.Y);
    fr_store(g + 16, p.Z);
    fr_store(g + 24, p.T);
}
// the point k_into_xy left at xy (x then y, plain), or its negative
ZK_DI EP ep_from_xy(const uint32_t* xy, bool negative) {
    Fr x = zkdev::to_mont(fr_load(xy));
    const Fr y = zkdev::to_mont(fr_load(xy + 8));
    if (negative) x = neg(x);
    return EP{x, y, Fr::one(), mul(x, y)};
}
// lane t's EP of the scan's LDS: [X Y Z T][word][lane]
ZK_DI void scan_st(uint32_t* lds, uint32_t t, const EP& v) {
#pragma unroll
    for (int w = 0; w < 8; w++) {
        lds[(0 * 8 + w) * LEDGER_SCAN_W + t] = v.X.l[w];
        lds[(1 * 8 + w) * LEDGER_SCAN_W + t] = v.Y.l[w];
        lds[(2 * 8 + w) * LEDGER_SCAN_W + t] = v.Z.l[w];
        lds[(3 * 8 + w) * LEDGER_SCAN_W + t] = v.T.l[w];
    }
}
ZK_DI EP scan_ld(const uint32_t* lds, uint32_t t) {
    EP r;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        r.X.l[w] = lds[(0 * 8 + w) * LEDGER_SCAN_W + t];
        r.Y.l[w] = lds[(1 * 8 + w) * LEDGER_SCAN_W + t];
        r.Z.l[w] = lds[(2 * 8 + w) * LEDGER_SCAN_W + t];
        r.T.l[w] = lds[(3 * 8 + w) * LEDGER_SCAN_W + t];
    }
    return r;
}
// The inclusive segmented scan of a workgroup (Kogge-Stone): reach = the lanes left of lane t, in this workgroup, that belong
// to its segment (<= t).  Before step d the lane holds the sum of the min(reach, d - 1) lanes to its left and its own; lane
// t - d is of its segment exactly when d <= reach, and then holds what continues that run.  Every lane of the workgroup calls.
ZK_DI EP block_scan(uint32_t* lds, uint32_t t, EP v, uint32_t reach, const Fr& d2) {
#pragma unroll 1
    for (uint32_t d = 1; d < LEDGER_SCAN_W; d <<= 1) {
        scan_st(lds, t, v);
        __syncthreads();
        const bool take = d <= reach;
        EP o = v;
        if (take) o = scan_ld(lds, t - d);
        __syncthreads();
        if (take) v = ext_add(o, v, d2);
    }
    return v;
}

// xy, st: k_into_xy's output for the points [slot 0 left, slot 0 right, .., op 0 left, op 0 right, ..].  off: n_slots + 1
// offsets of the slots into the slot-major order; perm: the op at each place of that order; slotv, flagv: by op.
// pre[c][j]: the exclusive prefix of place j inside its slot as far as this workgroup sees it; tot[c][s]: the same for the end
// of slot s, written by the workgroup that holds its last op; agg[c][b]: the inclusive value of the workgroup's last lane.
static __global__ void __launch_bounds__(LEDGER_SCAN_W)
k_ledger_scan(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* perm, const uint32_t* slotv, const uint32_t* flagv,
              uint32_t n_slots, uint32_t n_ops, uint32_t* pre, uint32_t* tot, uint32_t* agg) {
    ZK_SHARED uint32_t lds[4 * 8 * LEDGER_SCAN_W];
    const uint32_t t = threadIdx.x, c = blockIdx.y, b0 = blockIdx.x * LEDGER_SCAN_W, j = b0 + t;
    const bool live = j < n_ops;
    const Fr d2 = zkxt::jubjub_d2();
    EP v = zkxt::ep_neutral();
    uint32_t s = 0, reach = 0;
    if (live) {
        const uint32_t i = perm[j], fl = flagv[i];
        const size_t p = 2 * ((size_t)n_slots + i);
        s = slotv[i];
        if (!(fl & LEDGER_SKIP) && (st[p] | st[p + 1]) == 0) v = ep_from_xy(xy + (p + c) * 16, (fl & LEDGER_SUB) != 0);
        const uint32_t first = off[s] > b0 ? off[s] : b0;
        reach = j - first;
    }
    v = block_scan(lds, t, v, reach, d2);
    scan_st(lds, t, v);
    __syncthreads();
    if (live) {
        const EP e = reach ? scan_ld(lds, t - 1) : zkxt::ep_neutral();
        ep_store(pre + ((size_t)c * n_ops + j) * 32, e);
        if (j + 1 == off[s + 1]) ep_store(tot + ((size_t)c * n_slots + s) * 32, v);
    }
    if (t == LEDGER_SCAN_W - 1) ep_store(agg + ((size_t)c * gridDim.x + blockIdx.x) * 32, v);
}

// carry[c][b]: what the workgroups before b hold of the slot that is open where b begins (the identity for b = 0).
// cstart[b]: the last workgroup at or before b in which a slot starts (0 if none).  One workgroup per component walks the
// tails W at a time; the sum that runs into the next W waits in LDS.
static __global__ void __launch_bounds__(LEDGER_SCAN_W)
k_ledger_carry(const uint32_t* agg, const uint32_t* cstart, uint32_t n_blocks, uint32_t* carry) {
    ZK_SHARED uint32_t lds[4 * 8 * LEDGER_SCAN_W];
    const uint32_t t = threadIdx.x, c = blockIdx.y;
    const Fr d2 = zkxt::jubjub_d2();
    EP run = zkxt::ep_neutral();
    if (t == 0) ep_store(carry + (size_t)c * n_blocks * 32, run);
#pragma unroll 1
    for (uint32_t base = 0; base < n_blocks; base += LEDGER_SCAN_W) {
        const uint32_t b = base + t;
        const bool live = b < n_blocks;
        EP v = zkxt::ep_neutral();
        uint32_t reach = 0;
        bool open = false;   // the segment of b began before `base`: the running sum belongs to it
        if (live) {
            v = ep_load(agg + ((size_t)c * n_blocks + b) * 32);
            const uint32_t h = cstart[b];
            open = h < base;
            reach = b - (open ? base : h);
        }
        v = block_scan(lds, t, v, reach, d2);
        if (open) v = ext_add(run, v, d2);
        if (live && b + 1 < n_blocks) ep_store(carry + ((size_t)c * n_blocks + b + 1) * 32, v);
        scan_st(lds, t, v);
        __syncthreads();
        run = scan_ld(lds, LEDGER_SCAN_W - 1);
        __syncthreads();
    }
}

// Output point q: component q & 1 of slot q / 2 for q < 2 n_slots, else of the value op (q - 2 n_slots) / 2 met (pos: the
// op's place in the slot-major order).  enc: 8 words per output, Point::write of the affine sum; zero where the slot is refused.
static __global__ void __launch_bounds__(64)
k_ledger_encode(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* pos, const uint32_t* slotv, const uint32_t* pre,
                const uint32_t* tot, const uint32_t* carry, uint32_t n_slots, uint32_t n_ops, uint32_t n_blocks, uint32_t n_out, uint32_t* enc) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_out) return;
    const zkxt::Lds L{table + threadIdx.x};
    const uint32_t c = q & 1;
    uint32_t s, last = 0;   // last: the place whose workgroup's carry the sum lacks
    const uint32_t* src = nullptr;
    if (q < 2 * n_slots) {
        s = q >> 1;
        if (off[s + 1] > off[s]) {
            last = off[s + 1] - 1;
            src = tot + ((size_t)c * n_slots + s) * 32;
        }
    } else {
        const uint32_t i = (q - 2 * n_slots) >> 1;
        s = slotv[i];
        last = pos[i];
        src = pre + ((size_t)c * n_ops + last) * 32;
    }
    Fr y = Fr::zero();
    if ((st[2 * (size_t)s] | st[2 * (size_t)s + 1]) == 0) {
        const Fr d2 = zkxt::jubjub_d2();
        EP v = ep_from_xy(xy + (2 * (size_t)s + c) * 16, false);
        if (src) {
            EP sum = ep_load(src);
            const uint32_t b = last / LEDGER_SCAN_W;
            if (off[s] < b * LEDGER_SCAN_W) sum = ext_add(ep_load(carry + ((size_t)c * n_blocks + b) * 32), sum, d2);
            v = ext_add(v, sum, d2);
        }
        constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
        const Fr zi = zkxt::pow_windows(L, v.Z, EI);   // Z != 0: the addition law is complete on the prime-order subgroup
        y = zkxt::point_words(mul(v.X, zi), mul(v.Y, zi));
    }
    fr_store(enc + (size_t)q * 8, y);
}

// ---- host side
// status of a ciphertext from the IntoXY statuses of its points: 0, or (1 = left, 2 = right) | status << 6 of the first refused
inline uint8_t ct_status(uint32_t left, uint32_t right) { return left ? (uint8_t)(1u | (left << 6)) : right ? (uint8_t)(2u | (right << 6)) : 0; }

// the stable grouping of the ops by slot, slot_of(i) the slot of op i: off (n_slots + 1), perm (place -> op), pos (op -> place),
// and cstart, per workgroup of the scan the last one at or before it in which a slot starts (k_ledger_carry)
struct Grouping {
    std::vector<uint32_t> off, perm, pos, cstart;
    template <class SlotOf>
    Grouping(size_t n_slots, size_t n_ops, SlotOf&& slot_of)
        : off(n_slots + 1, 0), perm(n_ops), pos(n_ops), cstart((n_ops + LEDGER_SCAN_W - 1) / LEDGER_SCAN_W) {
        for (size_t i = 0; i < n_ops; i++) off[slot_of(i) + 1]++;
        for (size_t s = 0; s < n_slots; s++) off[s + 1] += off[s];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        for (size_t i = 0; i < n_ops; i++) {
            pos[i] = at[slot_of(i)]++;
            perm[pos[i]] = (uint32_t)i;
        }
        for (size_t b = 0, h = 0; b < cstart.size(); b++) {   // a slot starts in workgroup b: the slot of its last place starts at or after its first
            const size_t lastj = std::min(n_ops, (b + 1) * LEDGER_SCAN_W) - 1;
            if (off[slot_of(perm[lastj])] >= b * LEDGER_SCAN_W) h = b;
            cstart[b] = (uint32_t)h;
        }
    }
};

inline void point_write(const zkwit::JPoint& p, uint8_t out[32]) {   // edwards::Point::write
    const zkhost::Fr x = p.x.from_mont(), y = p.y.from_mont();
    memcpy(out, y.l, 32);
    if (x.l[0] & 1) out[31] |= 0x80;
}

// a decoded point, or its negative, in extended coordinates
inline zkwit::EPoint ext_signed(const zkwit::JPoint& p, bool negative) {
    zkwit::EPoint a = zkwit::to_ext(p);
    if (negative) {
        a.X = zkhost::Fr::zero() - a.X;
        a.T = zkhost::Fr::zero() - a.T;
    }
    return a;
}

// the device pointers the scan, the carry and the encoder share, named as the kernels' arguments
struct ScanBufs {
    const uint32_t *lxy, *lst, *off, *perm, *pos, *slotv, *flagv, *cstart;
    uint32_t *pre, *tot, *agg, *carry;
    uint32_t n_slots, n_ops, n_blocks;
};
inline void launch_scan(const ScanBufs& B) {
    if (!B.n_blocks) return;
    zkrt::ProfScope ps("ledger_scan");
    ZK_LAUNCH_SYNC(k_ledger_scan, dim3(B.n_blocks, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, B.lxy, B.lst, B.off, B.perm, B.slotv, B.flagv, B.n_slots,
                   B.n_ops, B.pre, B.tot, B.agg);
    ZK_LAUNCH_SYNC(k_ledger_carry, dim3(1, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)B.agg, B.cstart, B.n_blocks, B.carry);
}
inline void launch_encode(const ScanBufs& B, size_t n_out, uint32_t* enc) {
    zkrt::ProfScope ps("ledger_encode");
    ZK_LAUNCH(k_ledger_encode, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, zkrt::g_stream, B.lxy, B.lst, B.off, B.pos, B.slotv, (const uint32_t*)B.pre,
              (const uint32_t*)B.tot, (const uint32_t*)B.carry, B.n_slots, B.n_ops, B.n_blocks, (uint32_t)n_out, enc);
}

inline zk_status apply_host(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, uint8_t* slots_out, uint8_t* before_out,
                            uint8_t* slot_status_out, uint8_t* op_status_out) {
    const size_t np = 2 * (n_slots + n_ops);
    std::vector<zkwit::JPoint> pt(np);
    std::vector<uint32_t> st(np);
    auto encoding = [&](size_t p) -> const uint8_t* {
        return p < 2 * n_slots ? slots + p * 32 : (p & 1 ? ops[(p - 2 * n_slots) >> 1].right : ops[(p - 2 * n_slots) >> 1].left);
    };
    zkxt::into_xy_points(np, encoding, st.data(), pt.data());
    for (size_t s = 0; s < n_slots; s++) slot_status_out[s] = ct_status(st[2 * s], st[2 * s + 1]);
    for (size_t i = 0; i < n_ops; i++) op_status_out[i] = ct_status(st[2 * (n_slots + i)], st[2 * (n_slots + i) + 1]);
    const Grouping g(n_slots, n_ops, [&](size_t i) { return ops[i].slot; });
    // a thread's share: consecutive slots of about equal weight, a slot weighing one more than its ops
    const size_t weight = n_slots + n_ops;
    const unsigned nth = zkrt::host_threads(weight / 32 + 1, 64);
    auto work = [&](unsigned t) {
        std::vector<zkwit::EPoint> vals;
        std::vector<uint8_t*> dst;
        for (size_t s = 0; s < n_slots; s++) {
            const size_t w = s + g.off[s];
            if (w < weight * t / nth || w >= weight * (t + 1) / nth) continue;
            if (slot_status_out[s]) {
                memset(slots_out + s * 64, 0, 64);
                for (uint32_t j = g.off[s]; before_out && j < g.off[s + 1]; j++) memset(before_out + (size_t)g.perm[j] * 64, 0, 64);
                continue;
            }
            zkwit::EPoint cur[2] = {zkwit::to_ext(pt[2 * s]), zkwit::to_ext(pt[2 * s + 1])};
            for (uint32_t j = g.off[s]; j < g.off[s + 1]; j++) {
                const size_t i = g.perm[j];
                for (int c = 0; before_out && c < 2; c++) {
                    vals.push_back(cur[c]);
                    dst.push_back(before_out + i * 64 + 32 * c);
                }
                if (op_status_out[i] || (ops[i].flags & LEDGER_SKIP)) continue;
                for (int c = 0; c < 2; c++) cur[c] = zkwit::ext_add(cur[c], ext_signed(pt[2 * (n_slots + i) + c], (ops[i].flags & LEDGER_SUB) != 0));
            }
            for (int c = 0; c < 2; c++) {
                vals.push_back(cur[c]);
                dst.push_back(slots_out + s * 64 + 32 * c);
            }
        }
        std::vector<zkwit::JPoint> aff(vals.size());
        zkwit::batch_to_affine(vals.data(), aff.data(), vals.size());
        for (size_t k = 0; k < aff.size(); k++) point_write(aff[k], dst[k]);
    };
    zkrt::run_threads(nth, work);
    return ZK_OK;
}

inline zk_status apply_device(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, int device, uint8_t* slots_out,
                              uint8_t* before_out, uint8_t* slot_status_out, uint8_t* op_status_out) {
    ZK_TRY(zkrt::use_device(device));
    const size_t np = 2 * (n_slots + n_ops), n_out = 2 * n_slots + (before_out ? 2 * n_ops : 0);
    const size_t n_blocks = (n_ops + LEDGER_SCAN_W - 1) / LEDGER_SCAN_W;
    std::vector<uint8_t> pts(np * 32);
    if (n_slots) memcpy(pts.data(), slots, n_slots * 64);
    for (size_t i = 0; i < n_ops; i++) memcpy(&pts[(n_slots + i) * 64], ops[i].left, 64);
    static_assert(offsetof(zk_ledger_op, right) == offsetof(zk_ledger_op, left) + 32, "left | right");
    // behind the encodings: off | perm | pos | slotv | flagv | cstart; behind the statuses: enc | pre | tot | agg | carry
    const size_t meta_words = n_slots + 1 + 4 * n_ops + n_blocks;
    const size_t enc_bytes = n_out * 32, ep_bytes = 128;
    const size_t work_bytes = (2 * n_ops + 2 * n_slots + 4 * n_blocks) * ep_bytes;
    zkxt::IntoXyBufs bufs;
    ZK_TRY(zkxt::into_xy_on_device(pts.data(), np, &bufs, meta_words * 4, enc_bytes + work_bytes));
    // ... and while the decoder runs: the grouping
    const Grouping g(n_slots, n_ops, [&](size_t i) { return ops[i].slot; });
    std::vector<uint32_t> meta(meta_words);
    const size_t m_perm = n_slots + 1, m_pos = m_perm + n_ops, m_slotv = m_pos + n_ops, m_flagv = m_slotv + n_ops, m_cstart = m_flagv + n_ops;
    std::copy(g.off.begin(), g.off.end(), meta.begin());
    std::copy(g.perm.begin(), g.perm.end(), meta.begin() + m_perm);
    std::copy(g.pos.begin(), g.pos.end(), meta.begin() + m_pos);
    for (size_t i = 0; i < n_ops; i++) {
        meta[m_slotv + i] = ops[i].slot;
        meta[m_flagv + i] = ops[i].flags;
    }
    std::copy(g.cstart.begin(), g.cstart.end(), meta.begin() + m_cstart);
    uint32_t* d_meta = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(bufs.in.p) + np * 32);
    HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), meta_words * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    const uint32_t* d_xy = bufs.out.as<const uint32_t>();
    uint32_t* d_enc = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(bufs.out.p) + zkxt::into_xy_out_bytes(np));
    uint32_t *d_pre = d_enc + n_out * 8, *d_tot = d_pre + 2 * n_ops * 32, *d_agg = d_tot + 2 * n_slots * 32, *d_carry = d_agg + 2 * n_blocks * 32;
    const ScanBufs B{d_xy,  d_xy + np * 16, d_meta, d_meta + m_perm, d_meta + m_pos,    d_meta + m_slotv, d_meta + m_flagv, d_meta + m_cstart,
                     d_pre, d_tot,          d_agg,  d_carry,         (uint32_t)n_slots, (uint32_t)n_ops,  (uint32_t)n_blocks};
    launch_scan(B);
    launch_encode(B, n_out, d_enc);
    HIP_TRY(hipGetLastError());
    // one copy back: the statuses of all points, the padding up to the encodings, the encodings
    const size_t st_at = np * 64, back_bytes = zkxt::into_xy_out_bytes(np) - st_at + enc_bytes;
    std::vector<uint32_t> back(back_bytes / 4);
    HIP_TRY(hipMemcpyAsync(back.data(), static_cast<const uint8_t*>(bufs.out.p) + st_at, back_bytes, hipMemcpyDeviceToHost, zkrt::g_stream));
    HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    const uint8_t* enc = reinterpret_cast<const uint8_t*>(back.data()) + (zkxt::into_xy_out_bytes(np) - st_at);
    for (size_t s = 0; s < n_slots; s++) slot_status_out[s] = ct_status(back[2 * s], back[2 * s + 1]);
    for (size_t i = 0; i < n_ops; i++) op_status_out[i] = ct_status(back[2 * (n_slots + i)], back[2 * (n_slots + i) + 1]);
    memcpy(slots_out, enc, n_slots * 64);
    if (before_out) memcpy(before_out, enc + n_slots * 64, n_ops * 64);
    return ZK_OK;
}

// zk_elgamal_ledger_apply.  The host form for device < 0 or up to ZKAMD_INTO_XY_HOST_MAX points (read per call; the decode is
// over nine tenths of either form's work, so IntoXY's crossover, counted in points, is this entry's too).
inline zk_status apply(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, int device, uint8_t* slots_out,
                       uint8_t* before_out, uint8_t* slot_status_out, uint8_t* op_status_out) {
    if (!n_slots && !n_ops) return ZK_OK;
    if ((n_slots && (!slots || !slots_out || !slot_status_out)) || (n_ops && (!ops || !op_status_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n_slots + n_ops > (size_t)1 << 28) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^28 slots and ops in one call");
    for (size_t i = 0; i < n_ops; i++) {
        if (ops[i].slot >= n_slots) return fail(ZK_ERR_INVALID_ARGUMENT, "op " + std::to_string(i) + ": slot " + std::to_string(ops[i].slot) + " of " + std::to_string(n_slots));
        if (ops[i].flags & ~(LEDGER_SUB | LEDGER_SKIP)) return fail(ZK_ERR_INVALID_ARGUMENT, "op " + std::to_string(i) + ": unknown flag bits");
    }
    if (device < 0 || 2 * (n_slots + n_ops) <= zkxt::into_xy_host_max()) return apply_host(n_slots, slots, n_ops, ops, slots_out, before_out, slot_status_out, op_status_out);
    return apply_device(n_slots, slots, n_ops, ops, device, slots_out, before_out, slot_status_out, op_status_out);
}

}  // namespace zkledger
