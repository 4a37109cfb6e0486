// A block of anonymous transfers executed in one call (zk_anonymous_block_execute): what
//   anonymous_balances::anonymous_transfer (modules/anonymous-balances/src/lib.rs:23-82) does to storage for every extrinsic of
//   a block in order - ensure_signed, rollover of the twelve ring members (:37-39, :169-206), the nonce pool (:42, :65),
//   verify_anonymous_proof against the members' balances (modules/zk-system/src/lib.rs:118-165) and twelve
//   add_pending_transfer (:67-69, :209-229) - with the reference's verdict for every extrinsic and the state to store.
// The parts are those of block_exec.h (Keys32, Carve, Op, k_block_gather), k_into_xy and the ledger's three kernels, unchanged.
// What differs from the confidential block is that ONE verification batch is exact:
//   Transfers only ever add to PENDING slots; a balance changes only by rollover.  Whether account a rolls over is known from
//   signatures and stored bytes alone: rolled[a] = due[a] && (some extrinsic that passes steps 1 and 2 names a).  An extrinsic
//   that reaches step 5 has itself rolled every due member of its ring, so the balance it meets for member a is
//   rolled[a] ? balance + pending : balance - whatever its position in the block and whatever any verdict.  So every extrinsic
//   that passes steps 1 and 2, carries no refused point and no nonce of the CALLER's pool is verified in one batch, and one host
//   sweep in order applies steps 4 to 7; the only order dependence left is the nonce pool (a later twin of an accepted nonce is
//   NONCE_USED although its proof was checked).
// The device form:
//   1. Every DISTINCT 32-byte encoding - 27 per extrinsic (twelve keys, twelve lefts, the right, rvk, nonce), four per account,
//      g_epoch - through ONE k_into_xy launch; the statuses come back while the signature check runs.
//   2. k_ring_balance_xy: two lanes (left, right) per ROLLED ACCOUNT, not per ring member: ext_add(balance, pending), 1 / Z by
//      pow_windows over digits_inverse() (~360 dependent products), from_mont, plain little-endian x, y (16 words) into the table
//      of rolled balances.  A block of 1024 extrinsics names up to 12 288 accounts: 2 n_acc inversions instead of 24 n.
//      LDS: pow_windows' table only, [slot][word][lane], 16 x 8 x 64 words = 32 KB per 64-lane block, every lane in its own bank;
//      nothing in scratch memory.
//   3. The input rows are k_block_gather's copies, 52 lanes per extrinsic to verify: the table of rolled balances lies in
//      k_into_xy's output buffer behind the statuses, on a 64-byte step from its base, so a source index at or above
//      `roll_at` names a rolled balance and one below it a decoded point - the same kernel, the same base, no second copy kernel.
//   4. The rows cross the host once (3 328 bytes per extrinsic) into zkrt::verify_batch.
//   5. After the sweep ONE k_ledger_scan / k_ledger_carry with the final skip bits and k_ledger_encode over the slot outputs.
//      Slots and ops as INTEGRATION.md 8.13: slot 2a the balance, 2a + 1 the pending transfer; a rollover is two ops (the stored
//      pending added to the balance and subtracted from the pending slot), an accepted extrinsic twelve additions on pending slots.
// The host form (up to ZKAMD_INTO_XY_HOST_MAX distinct encodings, read per call) does the same work on the host threads and
// writes the same bytes; the verification always runs on the key's device.
// Only verify.cpp includes this header.  The data is public chain state: nothing here is constant-time.
#pragma once
#include "block_exec.h"

namespace zkblock {

constexpr uint32_t RING = ZK_ANONYMOUS_SIZE;                 // twelve members
constexpr uint32_t AX_POINTS = 2 * RING + 3;                 // the encodings of an extrinsic: keys, lefts, right, rvk, nonce
constexpr uint32_t AX_FIELDS = 4 * RING + 4, AX_INPUT_WORDS = 2 * AX_FIELDS * 8;
enum { AP_RIGHT = 2 * RING, AP_RVK, AP_NONCE };

// ---- device side
// Lane q: component q & 1 of rolled account q / 2.  src[2 q], src[2 q + 1]: the decoded points (indices into xy, k_into_xy's
// output) of that component of its balance and of its pending transfer.  out: 16 words per lane, x then y, plain little-endian.
static __global__ void __launch_bounds__(64)
k_ring_balance_xy(const uint32_t* xy, const uint32_t* src, uint32_t n_lanes, uint32_t* out) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_lanes) return;
    const zkxt::Lds L{table + threadIdx.x};
    const uint32_t b = src[2 * (size_t)q], p = src[2 * (size_t)q + 1];
    const EP v = ext_add(zkledger::ep_from_xy(xy + (size_t)b * 16, false), zkledger::ep_from_xy(xy + (size_t)p * 16, false), zkledger::edwards_2d());
    constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
    // Z != 0: both addends passed as_prime_order in k_into_xy (the host rolls readable accounts only), the prime-order points are
    // a subgroup, and the addition law is complete there
    const Fr zi = zkxt::pow_windows(L, v.Z, EI);
    uint32_t* o = out + (size_t)q * 16;
    zkledger::fr_store(o, zkdev::from_mont(mul(v.X, zi)));
    zkledger::fr_store(o + 8, zkdev::from_mont(mul(v.Y, zi)));
}

// ---- host side
// verify(n_v, proofs, inputs, ok): zkrt::verify_batch on the key with 104 inputs (verify.cpp hands it in)
template <class Verify>
inline zk_status execute_anonymous(int device, zkxt::IntoXyBufs* xybufs, zkrt::DevBuf* work, zkrt::PinBuf* pin, Verify&& verify, size_t n,
                                   const zk_anonymous_xt* xts, const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n_acc,
                                   const zk_block_account* accounts, size_t n_pool, const uint8_t* nonce_pool, const uint8_t* g_epoch,
                                   zk_block_account* accounts_out, zk_block_verdict* verdicts_out, zk_block_stats* stats_out) {
    if ((n && (!xts || !verdicts_out || !g_epoch)) || (n_acc && (!accounts || !accounts_out)) || (n_pool && !nonce_pool) ||
        (n && sigs && !msg_offsets))
        return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (size_t)1 << 20 || n_acc > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^20 extrinsics or 2^24 accounts in one call");
    // ---- the accounts by key, the rings' accounts
    Keys32 acc_of(n_acc);   // (the index of a key is that of its account)
    for (size_t a = 0; a < n_acc; a++) {
        bool fresh;
        acc_of.put(accounts[a].enc_key, &fresh);
        if (!fresh) return fail(ZK_ERR_INVALID_ARGUMENT, "account " + std::to_string(a) + ": its key is that of an earlier account");
    }
    std::vector<uint32_t> ring(n * RING);
    for (size_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < RING; k++) {
            ring[i * RING + k] = acc_of.find(xts[i].enc_keys[k]);
            if (ring[i * RING + k] == NO_POINT)
                return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": key " + std::to_string(k) + " of its ring is not among the accounts");
        }
    if (sigs)   // (as redjubjub.h's check_offsets: before anything is launched)
        for (size_t i = 0; i < n; i++) {
            if (msg_offsets[i + 1] < msg_offsets[i]) return fail(ZK_ERR_INVALID_ARGUMENT, "msg_offsets decrease at " + std::to_string(i));
            if (msg_offsets[i + 1] > msg_offsets[i] && !msgs) return fail(ZK_ERR_INVALID_ARGUMENT, "msgs is null but message " + std::to_string(i) + " is not empty");
        }
    zk_block_stats stats = {0, 0, 0, 0};
    if (!n) {
        if (n_acc) memcpy(accounts_out, accounts, n_acc * sizeof(zk_block_account));
        if (stats_out) *stats_out = stats;
        return ZK_OK;
    }
    // ---- 1. the distinct encodings
    Keys32 D(n * AX_POINTS + n_acc * 4 + 1);
    std::vector<uint32_t> xp(n * AX_POINTS), ap(n_acc * 4);
    for (size_t i = 0; i < n; i++) {
        const zk_anonymous_xt& x = xts[i];
        uint32_t* p = &xp[i * AX_POINTS];
        for (uint32_t k = 0; k < RING; k++) {
            p[k] = D.put(x.enc_keys[k]);
            p[RING + k] = D.put(x.left_ciphertexts[k]);
        }
        p[AP_RIGHT] = D.put(x.right_ciphertext);
        p[AP_RVK] = D.put(x.rvk);
        p[AP_NONCE] = D.put(x.nonce);
    }
    size_t n_due = 0;
    for (size_t a = 0; a < n_acc; a++) {
        for (int k = 0; k < 2; k++) {
            ap[a * 4 + k] = D.put(accounts[a].balance + 32 * k);
            ap[a * 4 + 2 + k] = D.put(accounts[a].pending + 32 * k);
        }
        n_due += (accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) != 0;
    }
    const uint32_t ge = D.put(g_epoch);
    const size_t nd = D.size();
    stats.points_decoded = (uint32_t)nd;
    const char* e = getenv("ZKAMD_INTO_XY_HOST_MAX");
    const size_t host_max = e && *e ? (size_t)strtoull(e, nullptr, 10) : zkxt::INTO_XY_HOST_MAX;
    const bool on_host = nd <= host_max;
    ZK_TRY(zkrt::use_device(device));
    // the table of rolled balances: behind the statuses in the decoder's output, on the 64-byte step of a decoded point
    const size_t roll_at = (zkxt::into_xy_out_bytes(nd) + 63) / 64;
    std::vector<uint32_t> dst(nd);        // statuses of the decoded points
    std::vector<zkwit::JPoint> hpt;       // host form: the decoded points
    if (on_host) {
        hpt.resize(nd);
        const unsigned nth = zkrt::host_threads(nd, 64);
        auto decode = [&](unsigned t) {
            for (size_t p = nd * t / nth; p < nd * (t + 1) / nth; p++) {
                uint8_t xy[64];
                dst[p] = zkxt::into_xy_one(&D.enc[p * 32], xy);
                zkhost::Fr x, y;
                memcpy(x.l, xy, 32);
                memcpy(y.l, xy + 32, 32);
                hpt[p] = zkwit::JPoint{x.to_mont(), y.to_mont()};
            }
        };
        zkrt::run_threads(nth, decode);
    } else {
        ZK_TRY(zkxt::into_xy_on_device(D.enc.data(), nd, xybufs, 0, (roll_at + 2 * n_due) * 64 - zkxt::into_xy_out_bytes(nd)));
    }
    // ---- 2. slots and ops, while the decoder runs.  The first extrinsic to name a due account carries that account's rollover,
    // every extrinsic its twelve additions: the order of the ops depends on no verdict, only their skip bits do.
    const size_t n_slots = 2 * n_acc;
    std::vector<Op> ops;
    ops.reserve(RING * n + 2 * n_due);
    std::vector<uint32_t> first_add(n), roll_op(n_acc, NO_POINT);   // roll_op: the first of the account's two rollover ops
    for (size_t i = 0; i < n; i++) {
        const uint32_t* p = &xp[i * AX_POINTS];
        for (uint32_t k = 0; k < RING; k++) {
            const uint32_t a = ring[i * RING + k];
            if (!(accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) || roll_op[a] != NO_POINT) continue;
            roll_op[a] = (uint32_t)ops.size();
            ops.push_back(Op{2 * a, 0, ap[a * 4 + 2], ap[a * 4 + 3]});
            ops.push_back(Op{2 * a + 1, LEDGER_SUB, ap[a * 4 + 2], ap[a * 4 + 3]});
        }
        first_add[i] = (uint32_t)ops.size();
        for (uint32_t k = 0; k < RING; k++) ops.push_back(Op{2 * ring[i * RING + k] + 1, LEDGER_SKIP, p[RING + k], p[AP_RIGHT]});
    }
    const size_t n_ops = ops.size(), np = 2 * (n_slots + n_ops), n_blocks = (n_ops + LEDGER_SCAN_W - 1) / LEDGER_SCAN_W;
    // the grouping of the ops by slot, as ledger.h's
    std::vector<uint32_t> off(n_slots + 1, 0), perm(n_ops), pos(n_ops), cstart(n_blocks);
    {
        for (size_t j = 0; j < n_ops; j++) off[ops[j].slot + 1]++;
        for (size_t s = 0; s < n_slots; s++) off[s + 1] += off[s];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        for (size_t j = 0; j < n_ops; j++) {
            pos[j] = at[ops[j].slot]++;
            perm[pos[j]] = (uint32_t)j;
        }
        for (size_t b = 0, h = 0; b < n_blocks; b++) {
            const size_t lastj = std::min(n_ops, (b + 1) * LEDGER_SCAN_W) - 1;
            if (off[ops[perm[lastj]].slot] >= b * LEDGER_SCAN_W) h = b;
            cstart[b] = (uint32_t)h;
        }
    }
    // ---- the device form's workspace and the layout the ledger's kernels read
    Carve cv;
    const size_t w_lxy = cv.take(np * 16), w_lst = cv.take(np), w_src = cv.take(np), w_off = cv.take(n_slots + 1), w_perm = cv.take(n_ops),
                 w_pos = cv.take(n_ops), w_slotv = cv.take(n_ops), w_flagv = cv.take(n_ops), w_cstart = cv.take(n_blocks),
                 w_pre = cv.take(2 * n_ops * 32), w_tot = cv.take(2 * n_slots * 32), w_agg = cv.take(2 * n_blocks * 32),
                 w_carry = cv.take(2 * n_blocks * 32), w_enc = cv.take(2 * n_slots * 8), w_vsrc = cv.take(n * AX_FIELDS), w_rsrc = cv.take(4 * n_due),
                 w_inputs = cv.take(n * AX_INPUT_WORDS);
    uint32_t *dw = nullptr, *d_roll = nullptr;
    const uint32_t *d_xy = nullptr, *d_st = nullptr;
    std::vector<uint32_t> flagv(n_ops);
    for (size_t j = 0; j < n_ops; j++) flagv[j] = ops[j].flags;
    if (!on_host) {
        ZK_TRY(work->ensure(cv.words * 4));
        dw = work->as<uint32_t>();
        d_xy = xybufs->out.as<const uint32_t>();
        d_st = d_xy + nd * 16;
        d_roll = xybufs->out.as<uint32_t>() + roll_at * 16;
        // src | off | perm | pos | slotv lie side by side: one upload
        std::vector<uint32_t> up(w_flagv - w_src, 0);
        uint32_t* src = up.data();
        for (size_t a = 0; a < n_acc; a++)
            for (int k = 0; k < 4; k++) src[4 * a + k] = ap[a * 4 + k];
        for (size_t j = 0; j < n_ops; j++) {
            src[2 * (n_slots + j)] = ops[j].left;
            src[2 * (n_slots + j) + 1] = ops[j].right;
            up[w_slotv - w_src + j] = ops[j].slot;
        }
        std::copy(off.begin(), off.end(), up.begin() + (w_off - w_src));
        std::copy(perm.begin(), perm.end(), up.begin() + (w_perm - w_src));
        std::copy(pos.begin(), pos.end(), up.begin() + (w_pos - w_src));
        HIP_TRY(hipMemcpyAsync(dw + w_src, up.data(), up.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
        if (n_blocks) HIP_TRY(hipMemcpyAsync(dw + w_cstart, cstart.data(), n_blocks * 4, hipMemcpyHostToDevice, zkrt::g_stream));
        {
            zkrt::ProfScope ps("block_gather");
            ZK_LAUNCH(k_block_gather, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, zkrt::g_stream, d_xy, d_st, (const uint32_t*)(dw + w_src),
                      (uint32_t)np, dw + w_lxy, dw + w_lst);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst.data(), d_st, nd * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
    }
    // ---- step 1 of every extrinsic: the signatures (the check's kernels queue behind the decoder and the gather, its hashing
    // runs beside them)
    std::vector<uint8_t> sig_ok(n, 1), sig_why(n, 0);
    if (sigs) {
        std::vector<uint8_t> vks(n * 32);
        for (size_t i = 0; i < n; i++) memcpy(&vks[i * 32], xts[i].rvk, 32);
        ZK_TRY(zk_redjubjub_verify_batch(n, vks.data(), sigs, msgs, msg_offsets, device, sig_ok.data(), sig_why.data()));
        ZK_TRY(zkrt::use_device(device));
    }
    if (!on_host) HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    std::vector<uint8_t> named(n_acc, 0);   // by a dispatched extrinsic
    for (size_t i = 0; i < n; i++)
        if (sig_ok[i])
            for (uint32_t k = 0; k < RING; k++) named[ring[i * RING + k]] = 1;
    // ---- steps 2, 3 and 5 as far as they do not depend on the order: unreadable accounts, rollovers, refused points
    auto acc_bad = [&](uint32_t a) { return (dst[ap[a * 4]] | dst[ap[a * 4 + 1]] | dst[ap[a * 4 + 2]] | dst[ap[a * 4 + 3]]) != 0; };
    enum { OPEN = 255 };
    std::vector<uint8_t> verdict(n, OPEN), refusal(n, 0), rolled(n_acc, 0);
    // field k = 0 .. 51 of extrinsic i as a decoded point; NO_POINT for the balances (fields 25 .. 48: step 2 judged them)
    auto field_point = [&](size_t i, uint32_t k) -> uint32_t {
        const uint32_t* p = &xp[i * AX_POINTS];
        if (k < 2 * RING) return p[k];
        if (k < 4 * RING) return NO_POINT;
        return k == 4 * RING ? p[AP_RIGHT] : k == 4 * RING + 1 ? p[AP_RVK] : k == 4 * RING + 2 ? ge : p[AP_NONCE];
    };
    size_t n_open = 0;
    for (size_t i = 0; i < n; i++) {
        if (!sig_ok[i]) {
            verdict[i] = ZK_BLOCK_BAD_SIGNATURE;
            continue;
        }
        bool bad = false;
        for (uint32_t k = 0; k < RING && !bad; k++) bad = acc_bad(ring[i * RING + k]);
        if (bad) {
            verdict[i] = ZK_BLOCK_BAD_ACCOUNT;   // (the reference's rollover(e)? loop would have rolled the members before the unreadable one)
            continue;
        }
        for (uint32_t k = 0; k < RING; k++) rolled[ring[i * RING + k]] = 1;   // (of a due account: step 3 is reached)
        for (uint32_t k = 0; k < AX_FIELDS && !refusal[i]; k++) {
            const uint32_t p = field_point(i, k);
            if (p != NO_POINT && dst[p]) refusal[i] = (uint8_t)((k + 1) | (dst[p] << 6));
        }
        n_open++;
    }
    std::vector<uint32_t> roll_idx(n_acc, NO_POINT), rolled_list;   // an account's place in the table of rolled balances
    for (size_t a = 0; a < n_acc; a++) {
        rolled[a] = rolled[a] && (accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE);
        if (roll_op[a] != NO_POINT && !rolled[a]) flagv[roll_op[a]] |= LEDGER_SKIP, flagv[roll_op[a] + 1] |= LEDGER_SKIP;
        if (rolled[a]) {
            roll_idx[a] = (uint32_t)rolled_list.size();
            rolled_list.push_back((uint32_t)a);
        }
    }
    const size_t n_rolled = rolled_list.size();
    stats.rounds = n_open ? 1 : 0;
    // ---- the one batch: every open extrinsic with no refused point and no nonce of the caller's pool
    std::vector<uint8_t> pool(nd, 0);   // by decoded point: a nonce of the caller's pool that no extrinsic carries plays no part
    for (size_t k = 0; k < n_pool; k++) {
        const uint32_t p = D.find(nonce_pool + 32 * k);
        if (p != NO_POINT) pool[p] = 1;
    }
    std::vector<uint32_t> todo;
    for (size_t i = 0; i < n; i++)
        if (verdict[i] == OPEN && !refusal[i] && !pool[xp[i * AX_POINTS + AP_NONCE]]) todo.push_back((uint32_t)i);
    const size_t nv = todo.size();
    std::vector<uint8_t> checked(n, 0);
    if (nv) {
        std::vector<uint8_t> proofs(nv * 192), inputs, ok(nv, 0);
        for (size_t v = 0; v < nv; v++) memcpy(&proofs[v * 192], xts[todo[v]].proof, 192);
        uint8_t* in_rows;   // the device form's rows come back into page-locked memory
        if (on_host) {
            std::vector<zkwit::EPoint> vals(2 * n_rolled);
            for (size_t r = 0; r < n_rolled; r++)
                for (int c = 0; c < 2; c++)
                    vals[2 * r + c] = zkwit::ext_add(zkwit::to_ext(hpt[ap[rolled_list[r] * 4 + c]]), zkwit::to_ext(hpt[ap[rolled_list[r] * 4 + 2 + c]]));
            std::vector<zkwit::JPoint> aff(2 * n_rolled);
            zkwit::batch_to_affine(vals.data(), aff.data(), 2 * n_rolled);
            inputs.assign(nv * AX_INPUT_WORDS * 4, 0);
            in_rows = inputs.data();
            for (size_t v = 0; v < nv; v++) {
                const uint32_t i = todo[v];
                for (uint32_t k = 0; k < AX_FIELDS; k++) {
                    const uint32_t p = field_point(i, k);
                    const zkwit::JPoint* q;
                    if (p != NO_POINT) {
                        q = &hpt[p];
                    } else {
                        const uint32_t c = k >= 3 * RING, a = ring[i * RING + (k - (2 + c) * RING)];
                        q = rolled[a] ? &aff[2 * roll_idx[a] + c] : &hpt[ap[a * 4 + c]];
                    }
                    const zkhost::Fr x = q->x.from_mont(), y = q->y.from_mont();
                    memcpy(in_rows + (v * AX_FIELDS + k) * 64, x.l, 32);
                    memcpy(in_rows + (v * AX_FIELDS + k) * 64 + 32, y.l, 32);
                }
            }
        } else {
            ZK_TRY(pin->ensure(nv * AX_INPUT_WORDS * 4));
            in_rows = pin->as<uint8_t>();
            std::vector<uint32_t> vsrc(nv * AX_FIELDS), rsrc(4 * n_rolled);
            for (size_t r = 0; r < n_rolled; r++)
                for (int c = 0; c < 2; c++) {
                    rsrc[4 * r + 2 * c] = ap[rolled_list[r] * 4 + c];
                    rsrc[4 * r + 2 * c + 1] = ap[rolled_list[r] * 4 + 2 + c];
                }
            for (size_t v = 0; v < nv; v++) {
                const uint32_t i = todo[v];
                for (uint32_t k = 0; k < AX_FIELDS; k++) {
                    uint32_t p = field_point(i, k);
                    if (p == NO_POINT) {
                        const uint32_t c = k >= 3 * RING, a = ring[i * RING + (k - (2 + c) * RING)];
                        p = rolled[a] ? (uint32_t)(roll_at + 2 * roll_idx[a] + c) : ap[a * 4 + c];
                    }
                    vsrc[v * AX_FIELDS + k] = p;
                }
            }
            HIP_TRY(hipMemcpyAsync(dw + w_vsrc, vsrc.data(), vsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
            if (n_rolled) {
                HIP_TRY(hipMemcpyAsync(dw + w_rsrc, rsrc.data(), rsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
                zkrt::ProfScope ps("ring_balance_xy");
                ZK_LAUNCH(k_ring_balance_xy, dim3((unsigned)((2 * n_rolled + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_xy, (const uint32_t*)(dw + w_rsrc),
                          (uint32_t)(2 * n_rolled), d_roll);
            }
            {
                zkrt::ProfScope ps("block_gather");
                ZK_LAUNCH(k_block_gather, dim3((unsigned)((nv * AX_FIELDS + 255) / 256)), dim3(256), 0, zkrt::g_stream, d_xy, d_st,
                          (const uint32_t*)(dw + w_vsrc), (uint32_t)(nv * AX_FIELDS), dw + w_inputs, (uint32_t*)nullptr);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(in_rows, dw + w_inputs, nv * AX_INPUT_WORDS * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
            HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        }
        ZK_TRY(verify(nv, proofs.data(), in_rows, ok.data()));
        ZK_TRY(zkrt::use_device(device));
        stats.proofs_verified = (uint32_t)nv;
        for (size_t v = 0; v < nv; v++) checked[todo[v]] = (uint8_t)(1 + ok[v]);
    }
    // ---- the state of the host form: every named, readable account, rolled over where that happens
    std::vector<zkwit::EPoint> hbal, hpen;
    if (on_host) {
        hbal.resize(2 * n_acc);
        hpen.resize(2 * n_acc);
        for (size_t a = 0; a < n_acc; a++) {
            if (!named[a] || acc_bad((uint32_t)a)) continue;
            for (int c = 0; c < 2; c++) {
                hbal[2 * a + c] = zkwit::to_ext(hpt[ap[a * 4 + c]]);
                hpen[2 * a + c] = zkwit::to_ext(hpt[ap[a * 4 + 2 + c]]);
                if (rolled[a]) {
                    hbal[2 * a + c] = zkwit::ext_add(hbal[2 * a + c], hpen[2 * a + c]);
                    hpen[2 * a + c] = zkwit::ext_zero();
                }
            }
        }
    }
    // ---- the sweep, in order: steps 4 to 7
    for (size_t i = 0; i < n; i++) {
        if (verdict[i] != OPEN) continue;
        const uint32_t nonce = xp[i * AX_POINTS + AP_NONCE];
        if (pool[nonce])
            verdict[i] = ZK_BLOCK_NONCE_USED;
        else if (refusal[i])
            verdict[i] = ZK_BLOCK_REFUSED_POINT;
        else if (checked[i] != 2)   // (an open extrinsic with a free nonce and no refusal was in the batch)
            verdict[i] = ZK_BLOCK_INVALID_PROOF;
        else {
            verdict[i] = ZK_BLOCK_ACCEPTED;
            pool[nonce] = 1;
            for (uint32_t k = 0; k < RING; k++) {
                const Op& op = ops[first_add[i] + k];
                flagv[first_add[i] + k] &= ~LEDGER_SKIP;
                if (!on_host) continue;
                hpen[op.slot - 1] = zkwit::ext_add(hpen[op.slot - 1], zkwit::to_ext(hpt[op.left]));
                hpen[op.slot] = zkwit::ext_add(hpen[op.slot], zkwit::to_ext(hpt[op.right]));
            }
        }
    }
    // ---- the state to store
    std::vector<uint8_t> enc(n_slots * 64, 0);
    if (on_host) {
        std::vector<zkwit::EPoint> vals;
        std::vector<uint8_t*> to;
        for (size_t a = 0; a < n_acc; a++) {
            if (!named[a] || acc_bad((uint32_t)a)) continue;
            for (int c = 0; c < 2; c++) {
                vals.push_back(hbal[2 * a + c]);
                to.push_back(&enc[(2 * a) * 64 + 32 * c]);
                vals.push_back(hpen[2 * a + c]);
                to.push_back(&enc[(2 * a + 1) * 64 + 32 * c]);
            }
        }
        std::vector<zkwit::JPoint> aff(vals.size());
        zkwit::batch_to_affine(vals.data(), aff.data(), vals.size());
        for (size_t k = 0; k < aff.size(); k++) zkledger::point_write(aff[k], to[k]);
    } else {
        if (n_blocks) {
            HIP_TRY(hipMemcpyAsync(dw + w_flagv, flagv.data(), n_ops * 4, hipMemcpyHostToDevice, zkrt::g_stream));
            zkrt::ProfScope ps("ledger_scan");
            ZK_LAUNCH_SYNC(zkledger::k_ledger_scan, dim3((unsigned)n_blocks, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)(dw + w_lxy),
                           (const uint32_t*)(dw + w_lst), (const uint32_t*)(dw + w_off), (const uint32_t*)(dw + w_perm), (const uint32_t*)(dw + w_slotv),
                           (const uint32_t*)(dw + w_flagv), (uint32_t)n_slots, (uint32_t)n_ops, dw + w_pre, dw + w_tot, dw + w_agg);
            ZK_LAUNCH_SYNC(zkledger::k_ledger_carry, dim3(1, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)(dw + w_agg),
                           (const uint32_t*)(dw + w_cstart), (uint32_t)n_blocks, dw + w_carry);
        }
        {
            zkrt::ProfScope ps("ledger_encode");
            ZK_LAUNCH(zkledger::k_ledger_encode, dim3((unsigned)((2 * n_slots + 63) / 64)), dim3(64), 0, zkrt::g_stream, (const uint32_t*)(dw + w_lxy),
                      (const uint32_t*)(dw + w_lst), (const uint32_t*)(dw + w_off), (const uint32_t*)(dw + w_pos), (const uint32_t*)(dw + w_slotv),
                      (const uint32_t*)(dw + w_pre), (const uint32_t*)(dw + w_tot), (const uint32_t*)(dw + w_carry), (uint32_t)n_slots,
                      (uint32_t)n_ops, (uint32_t)n_blocks, (uint32_t)(2 * n_slots), dw + w_enc);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(enc.data(), dw + w_enc, n_slots * 64, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    }
    for (size_t a = 0; a < n_acc; a++) {
        zk_block_account out = accounts[a];
        if (named[a]) {
            if (acc_bad((uint32_t)a)) {
                memset(out.balance, 0, 64);
                memset(out.pending, 0, 64);
            } else {
                memcpy(out.balance, &enc[(2 * a) * 64], 64);
                memcpy(out.pending, &enc[(2 * a + 1) * 64], 64);
            }
            if (rolled[a]) out.flags |= ZK_BLOCK_ROLLED;
        }
        accounts_out[a] = out;
    }
    for (size_t i = 0; i < n; i++)
        verdicts_out[i] = zk_block_verdict{verdict[i], (uint8_t)(verdict[i] == ZK_BLOCK_BAD_SIGNATURE ? sig_why[i] : verdict[i] == ZK_BLOCK_REFUSED_POINT ? refusal[i] : 0), 0};
    if (stats_out) *stats_out = stats;
    return ZK_OK;
}

}  // namespace zkblock
