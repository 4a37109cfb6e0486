// A block of anonymous transfers executed in one call (zk_anonymous_block_execute): what
//   anonymous_balances::anonymous_transfer (modules/anonymous-balances/src/lib.rs:23-82) does to storage for every extrinsic of
//   a block in order - ensure_signed, rollover of the twelve ring members (:37-39, :169-206), the nonce pool (:42, :65),
//   verify_anonymous_proof against the members' balances (modules/zk-system/src/lib.rs:118-165) and twelve
//   add_pending_transfer (:67-69, :209-229) - with the reference's verdict for every extrinsic and the state to store.
// The frame is block_frame.h's.  What differs from the confidential block is that ONE verification batch is exact:
//   Transfers only ever add to PENDING slots; a balance changes only by rollover.  Whether account a rolls over is known from
//   signatures and stored bytes alone: rolled[a] = due[a] && (some extrinsic that passes steps 1 and 2 names a).  An extrinsic
//   that reaches step 5 has itself rolled every due member of its ring, so the balance it meets for member a is
//   rolled[a] ? balance + pending : balance - whatever its position in the block and whatever any verdict.  So every extrinsic
//   that passes steps 1 and 2, carries no refused point and no nonce of the CALLER's pool is verified in one batch, and one host
//   sweep in order applies steps 4 to 7; the only order dependence left is the nonce pool (a later twin of an accepted nonce is
//   NONCE_USED although its proof was checked).
// What is this module's:
//   1. The encodings of an extrinsic: 27 (twelve keys, twelve lefts, the right, rvk, nonce).
//   2. Its ops: twelve additions on pending slots, and the rollover pair at the first extrinsic that names a due account.
//   3. k_ring_balance_xy: two lanes (left, right) per ROLLED ACCOUNT, not per ring member: ext_add(balance, pending), 1 / Z by
//      pow_windows over digits_inverse() (~360 dependent products), from_mont, plain little-endian x, y (16 words) into the table
//      of rolled balances.  A block of 1024 extrinsics names up to 12 288 accounts: 2 n_acc inversions instead of 24 n.
//      LDS: pow_windows' table only, [slot][word][lane], 16 x 8 x 64 words = 32 KB per 64-lane block, every lane in its own bank;
//      nothing in scratch memory.
//   4. The table of rolled balances lies behind the decoded points - in k_into_xy's output buffer behind the statuses, on a
//      64-byte step from its base (the host form appends it to its points) - so a row's field table names a rolled balance by
//      an index at or above `roll_at` and a decoded point by one below it: the rows are k_block_gather's copies, 52 lanes per
//      extrinsic to verify, the same kernel, the same base, no second copy kernel.  They cross the host once (3 328 bytes per
//      extrinsic) into zkrt::verify_batch.
// The row staging is the frame's except device_rows: the ring's kernel runs before the gather and reads no scan.
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
    const EP v = ext_add(zkledger::ep_from_xy(xy + (size_t)b * 16, false), zkledger::ep_from_xy(xy + (size_t)p * 16, false), zkxt::jubjub_d2());
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
inline zk_status execute_anonymous(const BlockArgs& A, Verify&& verify, const zk_anonymous_xt* xts) {
    const size_t n = A.n, n_acc = A.n_acc;
    if (null_args(A, xts)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (size_t)1 << 20 || n_acc > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^20 extrinsics or 2^24 accounts in one call");
    Keys32 acc_of(n_acc);
    ZK_TRY(accounts_by_key(A, &acc_of));
    std::vector<uint32_t> ring(n * RING);
    for (size_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < RING; k++) {
            ring[i * RING + k] = acc_of.find(xts[i].enc_keys[k]);
            if (ring[i * RING + k] == NO_POINT)
                return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": key " + std::to_string(k) + " of its ring is not among the accounts");
        }
    ZK_TRY(check_messages(A));
    if (!n) {
        empty_block(A);
        return ZK_OK;
    }
    // ---- 1. the distinct encodings, and room for the table of rolled balances on the 64-byte step of a decoded point
    Decoded P(n * AX_POINTS + n_acc * 4 + 1);
    std::vector<uint32_t> xp(n * AX_POINTS);
    for (size_t i = 0; i < n; i++) {
        const zk_anonymous_xt& x = xts[i];
        uint32_t* p = &xp[i * AX_POINTS];
        for (uint32_t k = 0; k < RING; k++) {
            p[k] = P.D.put(x.enc_keys[k]);
            p[RING + k] = P.D.put(x.left_ciphertexts[k]);
        }
        p[AP_RIGHT] = P.D.put(x.right_ciphertext);
        p[AP_RVK] = P.D.put(x.rvk);
        p[AP_NONCE] = P.D.put(x.nonce);
    }
    collect_accounts(A, &P);
    size_t n_due = 0;
    for (size_t a = 0; a < n_acc; a++) n_due += (A.accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) != 0;
    const size_t roll_at = P.on_host ? P.nd : (zkxt::into_xy_out_bytes(P.nd) + 63) / 64;
    ZK_TRY(decode(A, &P, P.on_host ? 0 : (roll_at + 2 * n_due) * 64 - zkxt::into_xy_out_bytes(P.nd)));
    // ---- 2. slots and ops, while the decoder runs
    std::vector<Op> ops;
    ops.reserve(RING * n + 2 * n_due);
    std::vector<uint32_t> first_add(n), roll_op(n_acc, NO_POINT);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* p = &xp[i * AX_POINTS];
        for (uint32_t k = 0; k < RING; k++) push_rollover(A, P, ring[i * RING + k], &roll_op, &ops);
        first_add[i] = (uint32_t)ops.size();
        for (uint32_t k = 0; k < RING; k++) ops.push_back(Op{2 * ring[i * RING + k] + 1, LEDGER_SKIP, p[RING + k], p[AP_RIGHT]});
    }
    Layout L(A, std::move(ops), AX_FIELDS);
    const size_t w_rsrc = L.cv.take(4 * n_due);
    ZK_TRY(to_device(A, &P, &L));
    Judgement J(A);
    ZK_TRY(check_signatures(A, xts, P.on_host, &J));
    // ---- steps 2, 3 and 5 as far as they do not depend on the order: unreadable accounts, rollovers, refused points
    for (size_t i = 0; i < n; i++)
        if (J.sig_ok[i])
            for (uint32_t k = 0; k < RING; k++) J.named[ring[i * RING + k]] = 1;
    std::vector<uint8_t> rolled(n_acc, 0);
    // the field table of extrinsic i: keys, lefts, NO_POINT for the balances (fields 25 .. 48: step 2 judged them), the rest
    uint32_t field[AX_FIELDS];
    auto fields_of = [&](size_t i) {
        const uint32_t* p = &xp[i * AX_POINTS];
        std::copy(p, p + 2 * RING, field);
        std::fill(field + 2 * RING, field + 4 * RING, NO_POINT);
        const uint32_t rest[4] = {p[AP_RIGHT], p[AP_RVK], P.ge, p[AP_NONCE]};
        std::copy(rest, rest + 4, field + 4 * RING);
    };
    for (size_t i = 0; i < n; i++) {
        if (!J.sig_ok[i]) {
            J.verdict[i] = ZK_BLOCK_BAD_SIGNATURE;
            continue;
        }
        bool bad = false;
        for (uint32_t k = 0; k < RING && !bad; k++) bad = acc_bad(P, ring[i * RING + k]);
        if (bad) {
            J.verdict[i] = ZK_BLOCK_BAD_ACCOUNT;   // (the reference's rollover(e)? loop would have rolled the members before the unreadable one)
            continue;
        }
        for (uint32_t k = 0; k < RING; k++) rolled[ring[i * RING + k]] = 1;   // (of a due account: step 3 is reached)
        fields_of(i);
        J.refusal[i] = refusal_of(P, field, AX_FIELDS);
        J.n_open++;
    }
    std::vector<uint32_t> roll_idx(n_acc, NO_POINT), rolled_list;   // an account's place in the table of rolled balances
    for (size_t a = 0; a < n_acc; a++) {
        rolled[a] = rolled[a] && (A.accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE);
        if (roll_op[a] != NO_POINT && !rolled[a]) L.skip_pair(roll_op[a]);
        if (rolled[a]) {
            roll_idx[a] = (uint32_t)rolled_list.size();
            rolled_list.push_back((uint32_t)a);
        }
    }
    const size_t n_rolled = rolled_list.size();
    J.stats.rounds = J.n_open ? 1 : 0;
    // ---- the one batch: every open extrinsic with no refused point and no nonce of the caller's pool
    mark_pool(A, P, &J);
    Rows R{AX_FIELDS};
    R.checked.resize(n);
    for (size_t i = 0; i < n; i++)
        if (J.verdict[i] == OPEN && !J.refusal[i] && !J.pool[xp[i * AX_POINTS + AP_NONCE]]) R.todo.push_back((uint32_t)i);
    const size_t nv = R.todo.size();
    if (nv) {
        ZK_TRY(begin_rows(A, P, xts, &R));
        for (size_t v = 0; v < nv; v++) {
            const uint32_t i = R.todo[v];
            fields_of(i);
            for (uint32_t k = 2 * RING; k < 4 * RING; k++) {   // component c of the balance member k - (2 + c) RING meets
                const uint32_t c = k >= 3 * RING, a = ring[i * RING + (k - (2 + c) * RING)];
                field[k] = rolled[a] ? (uint32_t)(roll_at + 2 * roll_idx[a] + c) : P.ap[a * 4 + c];
            }
            std::copy(field, field + AX_FIELDS, &R.vsrc[v * AX_FIELDS]);
        }
        if (P.on_host) {
            std::vector<zkwit::EPoint> vals(2 * n_rolled);
            for (size_t r = 0; r < n_rolled; r++)
                for (int c = 0; c < 2; c++)
                    vals[2 * r + c] = zkwit::ext_add(zkwit::to_ext(P.hpt[P.ap[rolled_list[r] * 4 + c]]), zkwit::to_ext(P.hpt[P.ap[rolled_list[r] * 4 + 2 + c]]));
            P.hpt.resize(roll_at + 2 * n_rolled);
            zkwit::batch_to_affine(vals.data(), &P.hpt[roll_at], 2 * n_rolled);
            host_rows(P, nullptr, &R);
        } else {
            std::vector<uint32_t> rsrc(4 * n_rolled);
            for (size_t r = 0; r < n_rolled; r++)
                for (int c = 0; c < 2; c++) {
                    rsrc[4 * r + 2 * c] = P.ap[rolled_list[r] * 4 + c];
                    rsrc[4 * r + 2 * c + 1] = P.ap[rolled_list[r] * 4 + 2 + c];
                }
            HIP_TRY(hipMemcpyAsync(L.dw + L.w_vsrc, R.vsrc.data(), R.vsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
            if (n_rolled) {
                HIP_TRY(hipMemcpyAsync(L.dw + w_rsrc, rsrc.data(), rsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
                zkrt::ProfScope ps("ring_balance_xy");
                ZK_LAUNCH(k_ring_balance_xy, dim3((unsigned)((2 * n_rolled + 63) / 64)), dim3(64), 0, zkrt::g_stream, P.d_xy, (const uint32_t*)(L.dw + w_rsrc),
                          (uint32_t)(2 * n_rolled), A.xybufs->out.as<uint32_t>() + roll_at * 16);
            }
            gather_rows(P, L, R);
            ZK_TRY(fetch_rows(L, R));
        }
        ZK_TRY(verify_rows(A, verify, &R, &J));
    }
    HostAccounts H;
    host_accounts(A, P, J, rolled, &H);
    // ---- the sweep, in order: steps 4 to 7
    for (size_t i = 0; i < n; i++) {
        if (J.verdict[i] != OPEN) continue;
        const uint32_t nonce = xp[i * AX_POINTS + AP_NONCE];
        if (J.pool[nonce])
            J.verdict[i] = ZK_BLOCK_NONCE_USED;
        else if (J.refusal[i])
            J.verdict[i] = ZK_BLOCK_REFUSED_POINT;
        else if (R.checked[i] != 2)   // (an open extrinsic with a free nonce and no refusal was in the batch)
            J.verdict[i] = ZK_BLOCK_INVALID_PROOF;
        else {
            J.verdict[i] = ZK_BLOCK_ACCEPTED;
            J.pool[nonce] = 1;
            for (uint32_t k = 0; k < RING; k++) {
                const Op& op = L.ops[first_add[i] + k];
                L.flagv[first_add[i] + k] &= ~LEDGER_SKIP;
                if (!P.on_host) continue;
                H.pen[op.slot - 1] = zkwit::ext_add(H.pen[op.slot - 1], zkwit::to_ext(P.hpt[op.left]));
                H.pen[op.slot] = zkwit::ext_add(H.pen[op.slot], zkwit::to_ext(P.hpt[op.right]));
            }
        }
    }
    // ---- the state to store
    std::vector<uint8_t> enc;
    ZK_TRY(stored_state(A, P, L, J, H, &enc));
    write_accounts(A, P, J, enc.data(), [&](size_t a) { return rolled[a] ? ZK_BLOCK_ROLLED : 0; });
    write_verdicts(A, P, &J);
    return ZK_OK;
}

}  // namespace zkblock
