// A block of encrypted-asset extrinsics executed in one call (zk_asset_block_execute): what the three dispatch functions of
//   modules/encrypted-assets/src/lib.rs - issue (:32-83), confidential_transfer (:86-164), destroy (:167-215) - do to storage for
//   every extrinsic of a block in order, with the reference's verdict for each, the accounts to store, the ids assigned and
//   the ciphertexts an issue creates and a destroy takes.
// The frame is block_frame.h's, a transfer's encodings, field table and ops are block_exec.h's.  What is this module's:
//   1. A scan that can FORGET.  destroy `take`s both stored ciphertexts: a slot's value after it is nothing plus the later ops,
//      whatever it held.  The ledger's segmented scan can only add, so an op flag LEDGER_CLEAR joins the two public ones (it
//      is internal: zk_elgamal_ledger_apply still refuses the bit).  A live CLEAR - neither skipped nor refused - adds nothing
//      and cuts the chain: the scan runs over pairs (cut, P) with (ca, A) . (cb, B) = cb ? (1, B) : (ca, A + B), which is
//      associative.  No select enters the point arithmetic, because block_scan already takes a `reach`: a lane's reach ends at
//      the later of its slot's first place in the workgroup and the last live CLEAR at or before it, and that last CLEAR is an
//      inclusive max-scan of one word per lane (place + 1, or 0), 8 steps in LDS beside the 8 ext_add steps of the points.  A
//      CLEAR of the slot before is ignored by the max with the slot's first place.
//        k_asset_scan     as k_ledger_scan, and a cut word for every place's exclusive prefix, every slot's total and the
//                         workgroup's tail: the chain was cut inside this workgroup
//        k_asset_carry    as k_ledger_carry over the tails: a workgroup's reach ends at the last workgroup at or before it whose
//                         tail is cut, the running sum between two passes of W applies only where no cut lies since the pass
//                         began; it writes, per workgroup, the carried sum and whether the carried chain holds a CLEAR
//        k_asset_encode, k_asset_balance_xy   as k_ledger_encode / k_block_balance_xy: sum = the prefix; where that is not cut and
//                         the slot began before the workgroup, carry + prefix and the carry's cut; the slot's stored value is
//                         added only to a chain that is not cut (so a slot whose stored value cannot be read has a value again
//                         after a CLEAR).  The encoder also writes the values that LISTED ops meet - what a destroy takes.
//      LDS: scan and carry keep one EP and one word per lane, 4 x 32 x W + 4 x W bytes; the two consumers pow_windows' table,
//      16 x 32 x 64 bytes.  Nothing in scratch memory.  The max-scan stays in LDS (no cross-lane instruction): it is 16
//      barriers and 8 word compares beside 72 field products, and the same source runs under the emulation build.
//   2. Slots and ops, laid out before any verdict is known (only the skip bits move): a transfer's three ops, the rollover pair
//      at the first TRANSFER that names a due account, a skipped CLEAR on both slots of its account for every destroy.
//   3. The rounds of block_exec.h with two more rules.  Issues and destroys take no balance from the ledger: only a still-open
//      nonce twin before them holds them, and their proofs are verified once.  A transfer is also held when an earlier destroy
//      of its sender's account is held or was accepted in this sweep.  A rollover pair is skipped when the account does not
//      roll, and when an ACCEPTED destroy of the account precedes the transfer that rolls it: it then moves nothing (the
//      pending transfer it would move was taken).  While such a destroy is open the pair is live - the hypothesis of a round
//      is that every still-open predecessor is rejected.  ONE round for a block in which no account sends twice and no destroy
//      precedes a transfer from its account.
//   4. Asset ids are assigned in one pass over the final verdicts.  Nothing in the call depends on them: an account, transfer
//      or destroy with an id this call may assign is an argument error.
//   5. The host form is a sequential walk over the ops in extended coordinates (host_walk) under the skip bits as they stand -
//      a CLEAR forgets, so the frame's per-account sums do not serve - and the effects: what an issue creates, a destroy takes.
#pragma once
#include <unordered_map>
#include "block_exec.h"

namespace zkblock {

constexpr uint32_t LEDGER_CLEAR = 4;   // internal: a live op with this flag forgets the slot's stored value and every op before it
using zkledger::ep_load;
using zkledger::ep_store;

// ---- device side
// The inclusive max-scan of one word per lane over the workgroup (Kogge-Stone in LDS, w: W words).  Every lane calls.
ZK_DI uint32_t block_max_scan(uint32_t* w, uint32_t t, uint32_t m) {
#pragma unroll 1
    for (uint32_t d = 1; d < LEDGER_SCAN_W; d <<= 1) {
        w[t] = m;
        __syncthreads();
        const uint32_t o = t >= d ? w[t - d] : 0;
        __syncthreads();
        m = o > m ? o : m;
    }
    return m;
}

// The arguments of k_ledger_scan, and cut: n_ops + n_slots + n_blocks words - whether the chain behind pre[.][j], tot[.][s],
// agg[.][b] was cut by a live CLEAR inside this workgroup (the same for both components: component 0 writes them).
static __global__ void __launch_bounds__(LEDGER_SCAN_W)
k_asset_scan(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* perm, const uint32_t* slotv, const uint32_t* flagv,
             uint32_t n_slots, uint32_t n_ops, uint32_t* pre, uint32_t* tot, uint32_t* agg, uint32_t* cut) {
    ZK_SHARED uint32_t lds[4 * 8 * LEDGER_SCAN_W];
    ZK_SHARED uint32_t clr[LEDGER_SCAN_W];
    const uint32_t t = threadIdx.x, c = blockIdx.y, b0 = blockIdx.x * LEDGER_SCAN_W, j = b0 + t;
    const bool live = j < n_ops;
    const Fr d2 = zkxt::jubjub_d2();
    EP v = zkxt::ep_neutral();
    uint32_t s = 0, first = b0, m = 0;   // first: the slot's first place in this workgroup; m: place + 1 of a live CLEAR
    if (live) {
        const uint32_t i = perm[j], fl = flagv[i];
        const size_t p = 2 * ((size_t)n_slots + i);
        s = slotv[i];
        if (!(fl & LEDGER_SKIP) && (st[p] | st[p + 1]) == 0) {
            if (fl & LEDGER_CLEAR)
                m = j + 1;
            else
                v = zkledger::ep_from_xy(xy + (p + c) * 16, (fl & LEDGER_SUB) != 0);
        }
        if (off[s] > b0) first = off[s];
    }
    const uint32_t cm = block_max_scan(clr, t, m);   // place + 1 of the last live CLEAR at or before this lane, 0 if none
    const bool cut_here = live && cm > first;        // (a CLEAR before `first` belongs to another slot)
    const uint32_t reach = live ? j - (cut_here ? cm - 1 : first) : 0;
    v = zkledger::block_scan(lds, t, v, reach, d2);
    zkledger::scan_st(lds, t, v);
    clr[t] = cm;
    __syncthreads();
    uint32_t *cut_pre = cut, *cut_tot = cut + n_ops, *cut_agg = cut_tot + n_slots;
    if (live) {
        const bool inner = j > first;   // lane t - 1 holds the slot's place before this one
        const EP e = inner ? zkledger::scan_ld(lds, t - 1) : zkxt::ep_neutral();
        ep_store(pre + ((size_t)c * n_ops + j) * 32, e);
        if (c == 0) cut_pre[j] = inner && clr[t - 1] > first;
        if (j + 1 == off[s + 1]) {
            ep_store(tot + ((size_t)c * n_slots + s) * 32, v);
            if (c == 0) cut_tot[s] = cut_here;
        }
    }
    if (t == LEDGER_SCAN_W - 1) {
        ep_store(agg + ((size_t)c * gridDim.x + blockIdx.x) * 32, v);
        if (c == 0) cut_agg[blockIdx.x] = cut_here;
    }
}

// The arguments of k_ledger_carry, cut_agg (k_asset_scan's tail words) and cut_carry[b]: the chain carry[.][b] holds a CLEAR.
static __global__ void __launch_bounds__(LEDGER_SCAN_W)
k_asset_carry(const uint32_t* agg, const uint32_t* cut_agg, const uint32_t* cstart, uint32_t n_blocks, uint32_t* carry, uint32_t* cut_carry) {
    ZK_SHARED uint32_t lds[4 * 8 * LEDGER_SCAN_W];
    ZK_SHARED uint32_t clr[LEDGER_SCAN_W];
    const uint32_t t = threadIdx.x, c = blockIdx.y;
    const Fr d2 = zkxt::jubjub_d2();
    EP run = zkxt::ep_neutral();
    uint32_t run_cut = 0;   // workgroup + 1 of the last cut tail of the passes so far
    if (t == 0) {
        ep_store(carry + (size_t)c * n_blocks * 32, run);
        if (c == 0) cut_carry[0] = 0;
    }
#pragma unroll 1
    for (uint32_t base = 0; base < n_blocks; base += LEDGER_SCAN_W) {
        const uint32_t b = base + t;
        const bool live = b < n_blocks;
        EP v = zkxt::ep_neutral();
        uint32_t h = 0, m = 0;
        if (live) {
            v = ep_load(agg + ((size_t)c * n_blocks + b) * 32);
            h = cstart[b];
            if (cut_agg[b]) m = b + 1;
        }
        uint32_t cm = block_max_scan(clr, t, m);
        if (run_cut > cm) cm = run_cut;
        const bool is_cut = live && cm > h;             // a cut tail at or after the workgroup in which the slot starts
        const uint32_t start = is_cut ? cm - 1 : h;     // the chain of b begins with this workgroup's tail
        const bool open = live && start < base;         // ... before this pass: the running sum belongs to it
        const uint32_t reach = live ? b - (open ? base : start) : 0;
        v = zkledger::block_scan(lds, t, v, reach, d2);
        if (open) v = ext_add(run, v, d2);
        if (live && b + 1 < n_blocks) {
            ep_store(carry + ((size_t)c * n_blocks + b + 1) * 32, v);
            if (c == 0) cut_carry[b + 1] = is_cut;
        }
        zkledger::scan_st(lds, t, v);
        clr[t] = cm;
        __syncthreads();
        run = zkledger::scan_ld(lds, LEDGER_SCAN_W - 1);
        run_cut = clr[LEDGER_SCAN_W - 1];
        __syncthreads();
    }
}

// The value at a place of slot s from what the scan left: *v = [stored value +] [carry +] prefix.  src, src_cut: the prefix
// or total of the place `last` and its cut word (src == nullptr: a slot without ops).  false: the value cannot be read (the
// stored value is refused and no CLEAR lies before the place).
ZK_DI bool asset_value(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* carry, const uint32_t* cut_carry, uint32_t n_blocks,
                       uint32_t s, uint32_t c, uint32_t last, const uint32_t* src, uint32_t src_cut, EP* v) {
    const Fr d2 = zkxt::jubjub_d2();
    const bool readable = (st[2 * (size_t)s] | st[2 * (size_t)s + 1]) == 0;
    if (!src) {
        if (readable) *v = zkledger::ep_from_xy(xy + (2 * (size_t)s + c) * 16, false);
        return readable;
    }
    EP sum = ep_load(src);
    bool is_cut = src_cut != 0;
    const uint32_t b = last / LEDGER_SCAN_W;
    if (!is_cut && off[s] < b * LEDGER_SCAN_W) {
        sum = ext_add(ep_load(carry + ((size_t)c * n_blocks + b) * 32), sum, d2);
        is_cut = cut_carry[b] != 0;
    }
    if (!is_cut) {
        if (!readable) return false;
        sum = ext_add(zkledger::ep_from_xy(xy + (2 * (size_t)s + c) * 16, false), sum, d2);
    }
    *v = sum;
    return true;
}

// Output point q: component q & 1 of slot q / 2 for q < 2 n_slots, else of the value the op listv[(q - 2 n_slots) / 2] met
// (listv == nullptr: the op (q - 2 n_slots) / 2).  The other arguments as k_ledger_encode, cut and cut_carry as above.
static __global__ void __launch_bounds__(64)
k_asset_encode(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* pos, const uint32_t* slotv, const uint32_t* listv,
               const uint32_t* pre, const uint32_t* tot, const uint32_t* carry, const uint32_t* cut, const uint32_t* cut_carry, uint32_t n_slots,
               uint32_t n_ops, uint32_t n_blocks, uint32_t n_out, uint32_t* enc) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_out) return;
    const zkxt::Lds L{table + threadIdx.x};
    const uint32_t c = q & 1;
    uint32_t s, last = 0, src_cut = 0;
    const uint32_t* src = nullptr;
    if (q < 2 * n_slots) {
        s = q >> 1;
        if (off[s + 1] > off[s]) {
            last = off[s + 1] - 1;
            src = tot + ((size_t)c * n_slots + s) * 32;
            src_cut = cut[n_ops + s];
        }
    } else {
        const uint32_t k = (q - 2 * n_slots) >> 1, i = listv ? listv[k] : k;
        s = slotv[i];
        last = pos[i];
        src = pre + ((size_t)c * n_ops + last) * 32;
        src_cut = cut[last];
    }
    Fr y = Fr::zero();
    EP v;
    if (asset_value(xy, st, off, carry, cut_carry, n_blocks, s, c, last, src, src_cut, &v)) {
        constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
        const Fr zi = zkxt::pow_windows(L, v.Z, EI);   // Z != 0: a sum of prime-order points
        y = zkxt::point_words(mul(v.X, zi), mul(v.Y, zi));
    }
    zkledger::fr_store(enc + (size_t)q * 8, y);
}

// As k_block_balance_xy: lane q writes component q & 1 of the value the op opv[q / 2] meets into fields 7 and 8 of input row
// q / 2.  opv[q / 2] == NO_POINT (an issue or a destroy: the row carries the extrinsic's own enc_balance) leaves the row alone.
static __global__ void __launch_bounds__(64)
k_asset_balance_xy(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* pos, const uint32_t* slotv, const uint32_t* pre,
                   const uint32_t* carry, const uint32_t* cut, const uint32_t* cut_carry, const uint32_t* opv, uint32_t n_ops, uint32_t n_blocks,
                   uint32_t n_v, uint32_t* inputs) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= 2 * n_v) return;
    const uint32_t i = opv[q >> 1];
    if (i == NO_POINT) return;
    const zkxt::Lds L{table + threadIdx.x};
    const uint32_t c = q & 1, s = slotv[i], last = pos[i];
    Fr x = Fr::zero(), y = Fr::zero();
    EP v;
    if (asset_value(xy, st, off, carry, cut_carry, n_blocks, s, c, last, pre + ((size_t)c * n_ops + last) * 32, cut[last], &v)) {
        constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
        const Fr zi = zkxt::pow_windows(L, v.Z, EI);   // Z != 0: a sum of prime-order points
        x = zkdev::from_mont(mul(v.X, zi));
        y = zkdev::from_mont(mul(v.Y, zi));
    }
    uint32_t* o = inputs + (size_t)(q >> 1) * XT_INPUT_WORDS + (6 + c) * 16;
    zkledger::fr_store(o, x);
    zkledger::fr_store(o + 8, y);
}

// ---- host side
// the device pointers the scan and its consumers share: the ledger's, and the cut words
struct AssetScanBufs : zkledger::ScanBufs {
    uint32_t *cut, *cut_carry;
};
inline zk_status asset_scan(const AssetScanBufs& B) {
    if (!B.n_blocks) return ZK_OK;
    zkrt::ProfScope ps("asset_scan");
    ZK_LAUNCH_SYNC(k_asset_scan, dim3(B.n_blocks, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, B.lxy, B.lst, B.off, B.perm, B.slotv, B.flagv, B.n_slots,
                   B.n_ops, B.pre, B.tot, B.agg, B.cut);
    ZK_LAUNCH_SYNC(k_asset_carry, dim3(1, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)B.agg,
                   (const uint32_t*)(B.cut + B.n_ops + B.n_slots), B.cstart, B.n_blocks, B.carry, B.cut_carry);
    return ZK_OK;
}
inline void asset_encode(const AssetScanBufs& B, const uint32_t* listv, size_t n_out, uint32_t* enc) {
    zkrt::ProfScope ps("asset_encode");
    ZK_LAUNCH(k_asset_encode, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, zkrt::g_stream, B.lxy, B.lst, B.off, B.pos, B.slotv, listv,
              (const uint32_t*)B.pre, (const uint32_t*)B.tot, (const uint32_t*)B.carry, (const uint32_t*)B.cut, (const uint32_t*)B.cut_carry, B.n_slots,
              B.n_ops, B.n_blocks, (uint32_t)n_out, enc);
}
inline void asset_balance_xy(const AssetScanBufs& B, const uint32_t* opv, size_t nv, uint32_t* inputs) {
    zkrt::ProfScope ps("asset_balance_xy");
    ZK_LAUNCH(k_asset_balance_xy, dim3((unsigned)((2 * nv + 63) / 64)), dim3(64), 0, zkrt::g_stream, B.lxy, B.lst, B.off, B.pos, B.slotv,
              (const uint32_t*)B.pre, (const uint32_t*)B.carry, (const uint32_t*)B.cut, (const uint32_t*)B.cut_carry, opv, B.n_ops, B.n_blocks,
              (uint32_t)nv, inputs);
}

// zk_hook_ledger_apply_clear (test builds only): zk_elgamal_ledger_apply's arguments with LEDGER_CLEAR allowed among the flags,
// always through the four kernels above, so that the scan is tested at sizes no forged block reaches.  With before_out,
// k_asset_balance_xy forms the value every op meets as well, and the hook fails unless its x, y encode to k_asset_encode's bytes.
inline zk_status apply_clear(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, int device, uint8_t* slots_out, uint8_t* before_out,
                             uint8_t* slot_status_out, uint8_t* op_status_out) {
    if (!n_slots && !n_ops) return ZK_OK;
    if ((n_slots && (!slots || !slots_out || !slot_status_out)) || (n_ops && (!ops || !op_status_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n_slots + n_ops > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^24 slots and ops in one call");
    for (size_t i = 0; i < n_ops; i++) {
        if (ops[i].slot >= n_slots) return fail(ZK_ERR_INVALID_ARGUMENT, "op " + std::to_string(i) + ": slot " + std::to_string(ops[i].slot) + " of " + std::to_string(n_slots));
        if (ops[i].flags & ~(LEDGER_SUB | LEDGER_SKIP | LEDGER_CLEAR)) return fail(ZK_ERR_INVALID_ARGUMENT, "op " + std::to_string(i) + ": unknown flag bits");
    }
    ZK_TRY(zkrt::use_device(device < 0 ? 0 : device));
    const size_t np = 2 * (n_slots + n_ops), n_out = 2 * n_slots + (before_out ? 2 * n_ops : 0), n_rows = before_out ? n_ops : 0;
    const size_t n_blocks = (n_ops + LEDGER_SCAN_W - 1) / LEDGER_SCAN_W;
    std::vector<uint8_t> pts(np * 32);
    if (n_slots) memcpy(pts.data(), slots, n_slots * 64);
    for (size_t i = 0; i < n_ops; i++) memcpy(&pts[(n_slots + i) * 64], ops[i].left, 64);
    const zkledger::Grouping g(n_slots, n_ops, [&](size_t i) { return ops[i].slot; });
    Carve mc, wc;   // behind the encodings: the grouping; behind the statuses: what the kernels write
    const size_t m_off = mc.take(n_slots + 1), m_perm = mc.take(n_ops), m_pos = mc.take(n_ops), m_slotv = mc.take(n_ops), m_flagv = mc.take(n_ops),
                 m_cstart = mc.take(n_blocks), m_opv = mc.take(n_rows);
    const size_t w_enc = wc.take(n_out * 8), w_pre = wc.take(2 * n_ops * 32), w_tot = wc.take(2 * n_slots * 32), w_agg = wc.take(2 * n_blocks * 32),
                 w_carry = wc.take(2 * n_blocks * 32), w_cut = wc.take(n_ops + n_slots + n_blocks), w_ccut = wc.take(n_blocks),
                 w_rows = wc.take(n_rows * XT_INPUT_WORDS);
    zkxt::IntoXyBufs bufs;
    ZK_TRY(zkxt::into_xy_on_device(pts.data(), np, &bufs, mc.words * 4 + 16, wc.words * 4 + 16));
    std::vector<uint32_t> meta(mc.words, 0);
    uint32_t* m = meta.data();
    std::copy(g.off.begin(), g.off.end(), m + m_off);
    std::copy(g.perm.begin(), g.perm.end(), m + m_perm);
    std::copy(g.pos.begin(), g.pos.end(), m + m_pos);
    for (size_t i = 0; i < n_ops; i++) {
        m[m_slotv + i] = ops[i].slot;
        m[m_flagv + i] = ops[i].flags;
    }
    std::copy(g.cstart.begin(), g.cstart.end(), m + m_cstart);
    for (size_t i = 0; i < n_rows; i++) m[m_opv + i] = (uint32_t)i;
    uint32_t* d_meta = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(bufs.in.p) + (np * 32 + 15) / 16 * 16);
    HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    const uint32_t *d_xy = bufs.out.as<const uint32_t>(), *d_st = d_xy + np * 16;
    uint32_t* dw = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(bufs.out.p) + (zkxt::into_xy_out_bytes(np) + 15) / 16 * 16);
    const AssetScanBufs B{{d_xy, d_st, d_meta + m_off, d_meta + m_perm, d_meta + m_pos, d_meta + m_slotv, d_meta + m_flagv, d_meta + m_cstart, dw + w_pre,
                           dw + w_tot, dw + w_agg, dw + w_carry, (uint32_t)n_slots, (uint32_t)n_ops, (uint32_t)n_blocks},
                          dw + w_cut,
                          dw + w_ccut};
    ZK_TRY(asset_scan(B));
    asset_encode(B, nullptr, n_out, dw + w_enc);
    if (n_rows) asset_balance_xy(B, d_meta + m_opv, n_rows, dw + w_rows);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> stv(np), enc(n_out * 8), rows(n_rows * XT_INPUT_WORDS);
    HIP_TRY(hipMemcpyAsync(stv.data(), d_st, np * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
    HIP_TRY(hipMemcpyAsync(enc.data(), dw + w_enc, n_out * 32, hipMemcpyDeviceToHost, zkrt::g_stream));
    if (n_rows) HIP_TRY(hipMemcpyAsync(rows.data(), dw + w_rows, rows.size() * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
    HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    for (size_t i = 0; i < n_rows; i++)
        for (size_t c = 0; c < 2; c++) {
            const uint32_t* xyw = &rows[i * XT_INPUT_WORDS + (6 + c) * 16];
            uint32_t want[8];
            std::copy(xyw + 8, xyw + 16, want);
            want[7] |= (xyw[0] & 1u) << 31;
            if (memcmp(want, &enc[(2 * n_slots + 2 * i + c) * 8], 32))
                return fail(ZK_ERR_DEVICE, "op " + std::to_string(i) + ": k_asset_balance_xy and k_asset_encode differ on the value it meets");
        }
    for (size_t s = 0; s < n_slots; s++) slot_status_out[s] = zkledger::ct_status(stv[2 * s], stv[2 * s + 1]);
    for (size_t i = 0; i < n_ops; i++) op_status_out[i] = zkledger::ct_status(stv[2 * (n_slots + i)], stv[2 * (n_slots + i) + 1]);
    memcpy(slots_out, enc.data(), n_slots * 64);
    if (before_out) memcpy(before_out, enc.data() + n_slots * 16, n_ops * 64);
    return ZK_OK;
}

// Point::write(Point::read(e)) for an encoding k_into_xy accepted: e itself, except that x = 0 may have come with the sign bit
// set - y = 1, the identity (y = -1 has order two and was refused) - and is written without it
inline void canonical32(const uint8_t* e, uint8_t out[32]) {
    memcpy(out, e, 32);
    bool identity = e[0] == 1 && e[31] == 0x80;
    for (int k = 1; k < 31 && identity; k++) identity = e[k] == 0;
    if (identity) out[31] = 0;
}

// verify(n_v, proofs, inputs, ok): zkrt::verify_batch on the key with 22 inputs (verify.cpp hands it in)
template <class Verify>
inline zk_status execute_asset(const BlockArgs& A, Verify&& verify, const zk_confidential_xt* xts, const uint8_t* kinds, const uint32_t* asset_ids,
                               const uint32_t* account_asset_ids, uint32_t next_asset_id, zk_asset_effect* effects_out, uint32_t* next_asset_id_out) {
    const size_t n = A.n, n_acc = A.n_acc;
    const zk_block_account* accounts = A.accounts;
    if (null_args(A, xts) || (n && (!kinds || !asset_ids || !effects_out)) || (n_acc && !account_asset_ids) || !next_asset_id_out)
        return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (size_t)1 << 24 || n_acc > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^24 extrinsics or accounts in one call");
    uint64_t n_issue = 0;
    for (size_t i = 0; i < n; i++) {
        if (kinds[i] > ZK_ASSET_DESTROY) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": kind " + std::to_string(kinds[i]));
        n_issue += kinds[i] == ZK_ASSET_ISSUE;
    }
    if ((uint64_t)next_asset_id + n_issue > UINT32_MAX) return fail(ZK_ERR_INVALID_ARGUMENT, "next_asset_id and the issue extrinsics of the call exceed the id's range");
    auto assignable = [&](uint32_t id) { return id >= next_asset_id && (uint64_t)id < (uint64_t)next_asset_id + n_issue; };
    // ---- the accounts by (asset id, key), the extrinsics' accounts
    Keys32 key_of(n_acc);
    std::unordered_map<uint64_t, uint32_t> acc_of;   // (id, index of the key's bytes) -> account
    acc_of.reserve(2 * n_acc);
    for (size_t a = 0; a < n_acc; a++) {
        if (assignable(account_asset_ids[a]))
            return fail(ZK_ERR_INVALID_ARGUMENT, "account " + std::to_string(a) + ": asset id " + std::to_string(account_asset_ids[a]) + " may be assigned by this call");
        const uint64_t k = (uint64_t)account_asset_ids[a] << 32 | key_of.put(accounts[a].enc_key);
        if (!acc_of.emplace(k, (uint32_t)a).second)
            return fail(ZK_ERR_INVALID_ARGUMENT, "account " + std::to_string(a) + ": its asset id and key are those of an earlier account");
    }
    auto find_acc = [&](uint32_t id, const uint8_t* key) {
        const uint32_t k = key_of.find(key);
        if (k == NO_POINT) return NO_POINT;
        const auto it = acc_of.find((uint64_t)id << 32 | k);
        return it == acc_of.end() ? NO_POINT : it->second;
    };
    std::vector<uint32_t> acc_s(n, NO_POINT), acc_r(n, NO_POINT);
    for (size_t i = 0; i < n; i++) {
        if (kinds[i] == ZK_ASSET_ISSUE) continue;
        if (assignable(asset_ids[i]))
            return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": asset id " + std::to_string(asset_ids[i]) + " may be assigned by this call");
        acc_s[i] = find_acc(asset_ids[i], xts[i].enc_key_sender);
        if (acc_s[i] == NO_POINT)
            return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the asset id and the " + (kinds[i] == ZK_ASSET_DESTROY ? "owner" : "sender") +
                                                     "'s key are not among the accounts");
        if (kinds[i] == ZK_ASSET_DESTROY) continue;
        acc_r[i] = find_acc(asset_ids[i], xts[i].enc_key_recipient);
        if (acc_r[i] == NO_POINT) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the asset id and the recipient's key are not among the accounts");
    }
    ZK_TRY(check_messages(A));
    if (!n) {
        empty_block(A);
        *next_asset_id_out = next_asset_id;
        return ZK_OK;
    }
    // ---- 1. the distinct encodings: a transfer's eight per extrinsic, and the halves of enc_balance of an issue or destroy
    Decoded P(n * (XT_POINTS + 2) + n_acc * 4 + 1);
    std::vector<uint32_t> xp(n * XT_POINTS), eb(n * 2, NO_POINT);
    size_t n_destroy = 0;
    for (size_t i = 0; i < n; i++) {
        transfer_points(xts[i], &P.D, &xp[i * XT_POINTS]);
        if (kinds[i] == ZK_ASSET_TRANSFER) continue;
        eb[2 * i] = P.D.put(xts[i].enc_balance);
        eb[2 * i + 1] = P.D.put(xts[i].enc_balance + 32);
        n_destroy += kinds[i] == ZK_ASSET_DESTROY;
    }
    collect_accounts(A, &P);
    ZK_TRY(decode(A, &P, 0));
    const std::vector<uint32_t>& ap = P.ap;
    // ---- 2. slots and ops, while the decoder runs: the order of the ops depends on no verdict
    std::vector<Op> ops;
    ops.reserve(4 * n + 2 * n_acc);
    std::vector<uint32_t> first_op(n, NO_POINT), roll_op(n_acc, NO_POINT);   // first_op: a transfer's first subtraction, a destroy's first CLEAR
    std::vector<uint32_t> destroy_at(n, NO_POINT), listv;   // the place of a destroy among the destroys: its two CLEARs are listed for the encoder
    for (size_t i = 0; i < n; i++) {
        if (kinds[i] == ZK_ASSET_ISSUE) continue;
        const uint32_t s = acc_s[i];
        if (kinds[i] == ZK_ASSET_TRANSFER) {
            push_rollover(A, P, s, &roll_op, &ops);
            push_rollover(A, P, acc_r[i], &roll_op, &ops);
            first_op[i] = (uint32_t)ops.size();
            push_transfer(s, acc_r[i], &xp[i * XT_POINTS], &ops);
            continue;
        }
        first_op[i] = (uint32_t)ops.size();   // (the points of a CLEAR are read and judged like any op's: the account's own balance)
        ops.push_back(Op{2 * s, LEDGER_CLEAR | LEDGER_SKIP, ap[s * 4], ap[s * 4 + 1]});
        ops.push_back(Op{2 * s + 1, LEDGER_CLEAR | LEDGER_SKIP, ap[s * 4], ap[s * 4 + 1]});
        destroy_at[i] = (uint32_t)(listv.size() / 2);
        listv.push_back(first_op[i]);
        listv.push_back(first_op[i] + 1);
    }
    Layout L(A, std::move(ops), XT_FIELDS, listv.size());
    const size_t n_slots = L.n_slots, n_ops = L.n_ops, w_cut = L.cv.take(n_ops + n_slots + L.n_blocks), w_ccut = L.cv.take(L.n_blocks);
    ZK_TRY(to_device(A, &P, &L, listv));
    const AssetScanBufs B = P.on_host ? AssetScanBufs{} : AssetScanBufs{L.B, L.dw + w_cut, L.dw + w_ccut};
    Judgement J(A);
    ZK_TRY(check_signatures(A, xts, P.on_host, &J));
    // ---- what does not depend on the order: named and unreadable accounts, the transfer that rolls an account, refused points
    std::vector<uint8_t> taken(n_acc, 0);
    std::vector<uint32_t> roll_at(n_acc, NO_POINT);   // the first transfer that reaches step 3 and names the due account
    auto fields_of = [&](size_t i, uint32_t* field) {
        const uint32_t* p = &xp[i * XT_POINTS];
        if (kinds[i] == ZK_ASSET_TRANSFER) return transfer_fields(p, P.ge, field);
        // (issuer, issuer, total, total, enc_balance, ..): lib.rs:55-66, :189-200
        const uint32_t f[XT_FIELDS] = {p[P_SENDER], p[P_SENDER],   p[P_AMOUNT_SENDER], p[P_AMOUNT_SENDER], p[P_RANDOMNESS], p[P_FEE],
                                       eb[2 * i],   eb[2 * i + 1], p[P_RVK],           P.ge,               p[P_NONCE]};
        std::copy(f, f + XT_FIELDS, field);
    };
    for (size_t i = 0; i < n; i++) {
        if (!J.sig_ok[i]) {
            J.verdict[i] = ZK_BLOCK_BAD_SIGNATURE;
            continue;
        }
        if (kinds[i] != ZK_ASSET_ISSUE) {
            J.named[acc_s[i]] = 1;
            bool bad = acc_bad(P, acc_s[i]);
            if (kinds[i] == ZK_ASSET_TRANSFER) {
                J.named[acc_r[i]] = 1;
                bad = bad || acc_bad(P, acc_r[i]);
            }
            if (bad) {
                J.verdict[i] = ZK_BLOCK_BAD_ACCOUNT;
                continue;
            }
            if (kinds[i] == ZK_ASSET_TRANSFER)
                for (const uint32_t a : {acc_s[i], acc_r[i]})
                    if ((accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) && roll_at[a] == NO_POINT) roll_at[a] = (uint32_t)i;
        }
        uint32_t field[XT_FIELDS];
        fields_of(i, field);
        J.refusal[i] = refusal_of(P, field, XT_FIELDS);
        J.n_open++;
    }
    for (size_t a = 0; a < n_acc; a++)
        if (roll_op[a] != NO_POINT && roll_at[a] == NO_POINT) L.skip_pair(roll_op[a]);
    // ---- the host form: a walk over the ops in order under the skip bits as they stand; want[j] >= 0 keeps the value op j meets
    std::vector<zkwit::EPoint> hcur;
    std::vector<int32_t> want(P.on_host ? n_ops : 0, -1);
    auto host_walk = [&](std::vector<zkwit::EPoint>& met) {   // met[2 want[j] + c]
        hcur.assign(2 * n_slots, zkwit::ext_zero());
        for (size_t a = 0; a < n_acc; a++)
            if (J.named[a] && !acc_bad(P, (uint32_t)a))
                for (int k = 0; k < 4; k++) hcur[4 * a + k] = zkwit::to_ext(P.hpt[ap[a * 4 + k]]);
        for (size_t j = 0; j < n_ops; j++) {
            const Op& o = L.ops[j];
            for (int c = 0; want[j] >= 0 && c < 2; c++) met[2 * want[j] + c] = hcur[2 * o.slot + c];
            if (L.flagv[j] & LEDGER_SKIP) continue;
            for (int c = 0; c < 2; c++)
                hcur[2 * o.slot + c] = o.flags & LEDGER_CLEAR
                                           ? zkwit::ext_zero()
                                           : zkwit::ext_add(hcur[2 * o.slot + c], zkledger::ext_signed(P.hpt[c ? o.right : o.left], (o.flags & LEDGER_SUB) != 0));
        }
    };
    // ---- 3. the rounds
    mark_pool(A, P, &J);
    Rows R{XT_FIELDS};
    R.checked.resize(n);
    std::vector<uint8_t> held_acc(n_acc), moved_acc(n_acc);
    std::unordered_set<uint32_t> held_nonces;
    while (J.n_open) {
        J.stats.rounds++;
        R.todo.clear();
        for (size_t i = 0; i < n; i++) {
            if (kinds[i] == ZK_ASSET_TRANSFER) R.checked[i] = 0;   // (an issue's or a destroy's proof meets no balance of the ledger: verified once)
            if (J.verdict[i] == OPEN && !J.refusal[i] && !R.checked[i] && !J.pool[xp[i * XT_POINTS + P_NONCE]]) R.todo.push_back((uint32_t)i);
        }
        const size_t nv = R.todo.size();
        if (nv) {
            ZK_TRY(begin_rows(A, P, xts, &R));
            for (size_t v = 0; v < nv; v++) {
                fields_of(R.todo[v], &R.vsrc[v * XT_FIELDS]);
                R.opv[v] = kinds[R.todo[v]] == ZK_ASSET_TRANSFER ? first_op[R.todo[v]] : NO_POINT;
            }
            if (P.on_host) {
                std::fill(want.begin(), want.end(), -1);
                for (size_t v = 0; v < nv; v++)
                    if (R.opv[v] != NO_POINT) want[R.opv[v]] = (int32_t)v;
                std::vector<zkwit::EPoint> vals(2 * nv, zkwit::ext_zero());
                host_walk(vals);
                std::vector<zkwit::JPoint> aff(2 * nv);
                zkwit::batch_to_affine(vals.data(), aff.data(), 2 * nv);
                host_rows(P, aff.data(), &R);
            } else {
                ZK_TRY(upload_flags(L));
                ZK_TRY(asset_scan(B));
                ZK_TRY(device_rows(P, L, R, [&] { asset_balance_xy(B, L.dw + L.w_opv, nv, L.dw + L.w_inputs); }));
            }
            ZK_TRY(verify_rows(A, verify, &R, &J));
        }
        // the sweep, in order
        std::fill(held_acc.begin(), held_acc.end(), 0);
        std::fill(moved_acc.begin(), moved_acc.end(), 0);
        held_nonces.clear();
        for (size_t i = 0; i < n; i++) {
            if (J.verdict[i] != OPEN) continue;
            const uint32_t nonce = xp[i * XT_POINTS + P_NONCE], a = acc_s[i];
            const bool transfer = kinds[i] == ZK_ASSET_TRANSFER;
            bool hold = (transfer && held_acc[a]) || held_nonces.count(nonce);
            if (!hold) {
                if (J.pool[nonce])
                    J.verdict[i] = ZK_BLOCK_NONCE_USED;
                else if (J.refusal[i])
                    J.verdict[i] = ZK_BLOCK_REFUSED_POINT;
                else if ((transfer && moved_acc[a]) || !R.checked[i])
                    hold = true;   // its balance changed in this sweep: the next round verifies it against the new one
                else if (R.checked[i] == 1)
                    J.verdict[i] = ZK_BLOCK_INVALID_PROOF;
                else {
                    J.verdict[i] = ZK_BLOCK_ACCEPTED;
                    J.pool[nonce] = 1;
                    if (transfer) {
                        moved_acc[a] = 1;
                        for (uint32_t j = first_op[i]; j < first_op[i] + 3; j++) L.flagv[j] &= ~LEDGER_SKIP;
                    } else if (kinds[i] == ZK_ASSET_DESTROY) {
                        moved_acc[a] = taken[a] = 1;
                        L.flagv[first_op[i]] &= ~LEDGER_SKIP, L.flagv[first_op[i] + 1] &= ~LEDGER_SKIP;
                        // a rollover at a later transfer moves nothing: the pending transfer it would move was taken
                        if (roll_op[a] != NO_POINT && roll_at[a] != NO_POINT && roll_at[a] > i) L.skip_pair(roll_op[a]);
                    }
                }
            }
            if (hold) {
                if (a != NO_POINT) held_acc[a] = 1;
                held_nonces.insert(nonce);
            } else {
                J.n_open--;
            }
        }
    }
    // ---- 4. the state to store and what the destroys took: one more scan under the final skip bits
    const size_t n_enc = 2 * n_slots + 2 * listv.size();
    std::vector<uint8_t> enc(n_enc * 32, 0);
    if (P.on_host) {
        std::fill(want.begin(), want.end(), -1);
        for (size_t k = 0; k < listv.size(); k++) want[listv[k]] = (int32_t)k;
        std::vector<zkwit::EPoint> vals(2 * listv.size(), zkwit::ext_zero());
        host_walk(vals);
        vals.insert(vals.begin(), hcur.begin(), hcur.end());
        std::vector<zkwit::JPoint> aff(vals.size());
        zkwit::batch_to_affine(vals.data(), aff.data(), vals.size());
        for (size_t k = 0; k < aff.size(); k++) zkledger::point_write(aff[k], &enc[k * 32]);
    } else if (n_enc) {
        ZK_TRY(upload_flags(L));
        ZK_TRY(asset_scan(B));
        asset_encode(B, L.dw + L.w_list, n_enc, L.dw + L.w_enc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(enc.data(), L.dw + L.w_enc, n_enc * 32, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    }
    write_accounts(A, P, J, enc.data(), [&](size_t a) { return (roll_at[a] != NO_POINT ? ZK_BLOCK_ROLLED : 0) | (taken[a] ? ZK_BLOCK_TAKEN : 0); });
    write_verdicts(A, P, &J);
    uint32_t next_id = next_asset_id;
    for (size_t i = 0; i < n; i++) {
        zk_asset_effect& fx = effects_out[i];
        memset(&fx, 0, sizeof fx);
        fx.asset_id = kinds[i] == ZK_ASSET_ISSUE ? 0 : asset_ids[i];
        if (J.verdict[i] != ZK_BLOCK_ACCEPTED) continue;
        if (kinds[i] == ZK_ASSET_ISSUE) {
            fx.asset_id = next_id++;
            if (P.on_host) {
                zkledger::point_write(P.hpt[xp[i * XT_POINTS + P_AMOUNT_SENDER]], fx.first);
                zkledger::point_write(P.hpt[xp[i * XT_POINTS + P_RANDOMNESS]], fx.first + 32);
            } else {
                canonical32(xts[i].left_amount_sender, fx.first);
                canonical32(xts[i].right_randomness, fx.first + 32);
            }
        } else if (kinds[i] == ZK_ASSET_DESTROY) {
            memcpy(fx.first, &enc[(n_slots + 2 * destroy_at[i]) * 64], 64);
            memcpy(fx.second, &enc[(n_slots + 2 * destroy_at[i] + 1) * 64], 64);
        }
    }
    *next_asset_id_out = next_id;
    return ZK_OK;
}

}  // namespace zkblock
