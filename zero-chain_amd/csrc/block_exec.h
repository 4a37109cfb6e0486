// A block of confidential transfers executed in one call (zk_confidential_block_execute): what
//   encrypted_balances::confidential_transfer (modules/encrypted-balances/src/lib.rs:25-96) does to storage for every extrinsic
//   of a block in order - ensure_signed, rollover of sender and recipient (:133-170), the nonce pool (:49, :69),
//   verify_confidential_proof against the sender's balance AS IT STANDS (modules/zk-system/src/lib.rs:56-115), sub_enc_balance
//   and add_pending_transfer (:173-222) - with the reference's verdict for every extrinsic and the state to store.
// The frame is block_frame.h's: the distinct encodings, the ledger layout, the signature step, the rows of a batch, the state
// to store.  What is this module's:
//   1. The encodings of an extrinsic: eight (both keys, the three lefts, the randomness, rvk, nonce).
//   2. Its ops: two subtractions from the sender's balance and one addition to the recipient's pending transfer (INTEGRATION.md
//      8.13), and the rollover pair at the first extrinsic that names a due account.  The order of the ops does not depend on
//      any verdict, only their skip bits do; whether a rollover happens is known once the signatures and the stored ciphertexts
//      are judged.
//   3. Rounds.  Which balance extrinsic i meets depends on which earlier ones were accepted, and that on their proofs.  A round
//      scans with the skip bit on every op not yet accepted, then verifies, in one batch, every extrinsic whose verdict is open,
//      each against the balance it meets if every still-open predecessor is rejected.  A host sweep in order then settles every
//      extrinsic whose hypothesis held: no predecessor of the same sender was accepted in this sweep or is still open, and no
//      predecessor with the same nonce is still open.  The first open one always settles, so the loop ends.  A block in which no
//      sender has two extrinsics that reach the proof takes ONE round and verifies every proof at most once.
//   4. k_block_balance_xy: two lanes (left, right) per extrinsic to verify.  The balance it meets is slot value + carry + prefix
//      of its first subtraction, read as k_ledger_encode reads them, made affine by 1 / Z (pow_windows over digits_inverse(),
//      ~360 dependent products) and written as plain little-endian x, y straight into that extrinsic's public inputs 13-16.
//      There is no Point::write, no second read_point and no is_prime_order here: the slot's value and every addend passed
//      as_prime_order in k_into_xy, the prime-order points are a subgroup, so their sum is one of them - and the addition law is
//      complete there, so Z != 0.  The other eighteen inputs are k_block_gather's copies from the decoded table.
//      LDS: pow_windows' table, [slot][word][lane] as jubjub_dev.h, 16 x 8 x 64 words = 32 KB per 64-lane block, every lane in
//      its own bank; nothing in scratch memory.  Five blocks fit a CU's 160 KB; the kernel is latency-bound like its neighbours.
//      The inputs of a round cross the host once (704 bytes per extrinsic) into zkrt::verify_batch, which stages its own uploads.
// The host form keeps every account in extended coordinates and adds an accepted extrinsic's three ops to it in the sweep.
#pragma once
#include <unordered_set>
#include "block_frame.h"

namespace zkblock {

constexpr uint32_t XT_POINTS = 8, XT_FIELDS = 11, XT_INPUT_WORDS = 2 * XT_FIELDS * 8;
// the eight encodings of an extrinsic in the order they are collected, and the field of zk_confidential_verify_batch each is
enum { P_SENDER = 0, P_RECIPIENT, P_AMOUNT_SENDER, P_AMOUNT_RECIPIENT, P_RANDOMNESS, P_FEE, P_RVK, P_NONCE };

// ---- device side
// Lane q: component q & 1 of the balance extrinsic opv-entry q / 2 meets - the value of the slot of op opv[q / 2] just before
// that op.  xy, st, off, pos, slotv, pre, carry: as k_ledger_encode.  inputs: n_v rows of XT_INPUT_WORDS words; x and y go to
// fields 7 (left) and 8 (right).
static __global__ void __launch_bounds__(64)
k_block_balance_xy(const uint32_t* xy, const uint32_t* st, const uint32_t* off, const uint32_t* pos, const uint32_t* slotv, const uint32_t* pre,
                   const uint32_t* carry, const uint32_t* opv, uint32_t n_ops, uint32_t n_blocks, uint32_t n_v, uint32_t* inputs) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= 2 * n_v) return;
    const zkxt::Lds L{table + threadIdx.x};
    const uint32_t c = q & 1, i = opv[q >> 1], s = slotv[i], last = pos[i];
    Fr x = Fr::zero(), y = Fr::zero();
    if ((st[2 * (size_t)s] | st[2 * (size_t)s + 1]) == 0) {
        const Fr d2 = zkxt::jubjub_d2();
        EP sum = zkledger::ep_load(pre + ((size_t)c * n_ops + last) * 32);
        const uint32_t b = last / LEDGER_SCAN_W;
        if (off[s] < b * LEDGER_SCAN_W) sum = ext_add(zkledger::ep_load(carry + ((size_t)c * n_blocks + b) * 32), sum, d2);
        const EP v = ext_add(zkledger::ep_from_xy(xy + (2 * (size_t)s + c) * 16, false), sum, d2);
        constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
        const Fr zi = zkxt::pow_windows(L, v.Z, EI);   // Z != 0: a sum of prime-order points
        x = zkdev::from_mont(mul(v.X, zi));
        y = zkdev::from_mont(mul(v.Y, zi));
    }
    uint32_t* o = inputs + (size_t)(q >> 1) * XT_INPUT_WORDS + (6 + c) * 16;
    zkledger::fr_store(o, x);
    zkledger::fr_store(o + 8, y);
}

// ---- host side: a confidential transfer (the assets' transfers are the same)
inline void transfer_points(const zk_confidential_xt& x, Keys32* D, uint32_t* p) {
    const uint8_t* f[XT_POINTS] = {x.enc_key_sender, x.enc_key_recipient, x.left_amount_sender, x.left_amount_recipient,
                                   x.right_randomness, x.left_fee, x.rvk, x.nonce};
    for (uint32_t k = 0; k < XT_POINTS; k++) p[k] = D->put(f[k]);
}
// its row's field table; NO_POINT: the sender's balance as the extrinsic meets it
inline void transfer_fields(const uint32_t* p, uint32_t ge, uint32_t* field) {
    const uint32_t f[XT_FIELDS] = {p[P_SENDER], p[P_RECIPIENT], p[P_AMOUNT_SENDER], p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS], p[P_FEE],
                                   NO_POINT,    NO_POINT,       p[P_RVK],           ge,                    p[P_NONCE]};
    std::copy(f, f + XT_FIELDS, field);
}
// its three ops, skipped until it is accepted, from account s to account r
inline void push_transfer(uint32_t s, uint32_t r, const uint32_t* p, std::vector<Op>* ops) {
    ops->push_back(Op{2 * s, LEDGER_SUB | LEDGER_SKIP, p[P_AMOUNT_SENDER], p[P_RANDOMNESS]});
    ops->push_back(Op{2 * s, LEDGER_SUB | LEDGER_SKIP, p[P_FEE], p[P_RANDOMNESS]});
    ops->push_back(Op{2 * r + 1, LEDGER_SKIP, p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS]});
}

// verify(n_v, proofs, inputs, ok): zkrt::verify_batch on the key (verify.cpp hands it in: zk_vk is defined there)
template <class Verify>
inline zk_status execute(const BlockArgs& A, Verify&& verify, const zk_confidential_xt* xts) {
    const size_t n = A.n, n_acc = A.n_acc;
    if (null_args(A, xts)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (size_t)1 << 24 || n_acc > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^24 extrinsics or accounts in one call");
    Keys32 acc_of(n_acc);
    ZK_TRY(accounts_by_key(A, &acc_of));
    std::vector<uint32_t> acc_s(n), acc_r(n);
    for (size_t i = 0; i < n; i++) {
        acc_s[i] = acc_of.find(xts[i].enc_key_sender);
        acc_r[i] = acc_of.find(xts[i].enc_key_recipient);
        if (acc_s[i] == NO_POINT) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the sender's key is not among the accounts");
        if (acc_r[i] == NO_POINT) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the recipient's key is not among the accounts");
    }
    ZK_TRY(check_messages(A));
    if (!n) {
        empty_block(A);
        return ZK_OK;
    }
    // ---- 1. the distinct encodings.  A key, a g_epoch or a randomness that recurs is decoded once.
    Decoded P(n * XT_POINTS + n_acc * 4 + 1);
    std::vector<uint32_t> xp(n * XT_POINTS);
    for (size_t i = 0; i < n; i++) transfer_points(xts[i], &P.D, &xp[i * XT_POINTS]);
    collect_accounts(A, &P);
    ZK_TRY(decode(A, &P, 0));
    // ---- 2. slots and ops, while the decoder runs
    std::vector<Op> ops;
    ops.reserve(4 * n + 2 * n_acc);
    std::vector<uint32_t> first_sub(n), roll_op(n_acc, NO_POINT);
    for (size_t i = 0; i < n; i++) {
        push_rollover(A, P, acc_s[i], &roll_op, &ops);
        push_rollover(A, P, acc_r[i], &roll_op, &ops);
        first_sub[i] = (uint32_t)ops.size();
        push_transfer(acc_s[i], acc_r[i], &xp[i * XT_POINTS], &ops);
    }
    Layout L(A, std::move(ops), XT_FIELDS);
    ZK_TRY(to_device(A, &P, &L));
    Judgement J(A);
    ZK_TRY(check_signatures(A, xts, P.on_host, &J));
    // ---- steps 2 and 5 as far as they do not depend on the order: unreadable accounts, refused points
    for (size_t i = 0; i < n; i++)
        if (J.sig_ok[i]) J.named[acc_s[i]] = J.named[acc_r[i]] = 1;
    std::vector<uint8_t> rolled(n_acc, 0);
    uint32_t field[XT_FIELDS];
    for (size_t i = 0; i < n; i++) {
        if (!J.sig_ok[i]) {
            J.verdict[i] = ZK_BLOCK_BAD_SIGNATURE;
            continue;
        }
        if (acc_bad(P, acc_s[i]) || acc_bad(P, acc_r[i])) {
            J.verdict[i] = ZK_BLOCK_BAD_ACCOUNT;
            continue;
        }
        rolled[acc_s[i]] = rolled[acc_r[i]] = 1;   // (of a due account: step 3 is reached)
        transfer_fields(&xp[i * XT_POINTS], P.ge, field);
        J.refusal[i] = refusal_of(P, field, XT_FIELDS);
        J.n_open++;
    }
    for (size_t a = 0; a < n_acc; a++) {
        rolled[a] = rolled[a] && (A.accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE);
        if (roll_op[a] != NO_POINT && !rolled[a]) L.skip_pair(roll_op[a]);
    }
    HostAccounts H;
    host_accounts(A, P, J, rolled, &H);
    mark_pool(A, P, &J);
    // ---- 3. the rounds
    Rows R{XT_FIELDS};
    R.checked.resize(n);
    std::vector<uint8_t> held_sender(n_acc), moved_sender(n_acc);
    std::unordered_set<uint32_t> held_nonces;
    while (J.n_open) {
        J.stats.rounds++;
        R.todo.clear();
        for (size_t i = 0; i < n; i++)
            if (J.verdict[i] == OPEN && !J.refusal[i] && !J.pool[xp[i * XT_POINTS + P_NONCE]]) R.todo.push_back((uint32_t)i);
        const size_t nv = R.todo.size();
        std::fill(R.checked.begin(), R.checked.end(), 0);
        if (nv) {
            ZK_TRY(begin_rows(A, P, xts, &R));
            for (size_t v = 0; v < nv; v++) {
                transfer_fields(&xp[R.todo[v] * XT_POINTS], P.ge, &R.vsrc[v * XT_FIELDS]);
                R.opv[v] = first_sub[R.todo[v]];
            }
            if (P.on_host) {
                std::vector<zkwit::EPoint> vals(2 * nv);
                for (size_t v = 0; v < nv; v++)
                    for (int c = 0; c < 2; c++) vals[2 * v + c] = H.bal[2 * acc_s[R.todo[v]] + c];
                std::vector<zkwit::JPoint> aff(2 * nv);
                zkwit::batch_to_affine(vals.data(), aff.data(), 2 * nv);
                host_rows(P, aff.data(), &R);
            } else {
                ZK_TRY(upload_flags(L));
                zkledger::launch_scan(L.B);
                ZK_TRY(device_rows(P, L, R, [&] {
                    zkrt::ProfScope ps("block_balance_xy");
                    ZK_LAUNCH(k_block_balance_xy, dim3((unsigned)((2 * nv + 63) / 64)), dim3(64), 0, zkrt::g_stream, L.B.lxy, L.B.lst, L.B.off, L.B.pos, L.B.slotv,
                              (const uint32_t*)L.B.pre, (const uint32_t*)L.B.carry, (const uint32_t*)(L.dw + L.w_opv), L.B.n_ops, L.B.n_blocks, (uint32_t)nv,
                              L.dw + L.w_inputs);
                }));
            }
            ZK_TRY(verify_rows(A, verify, &R, &J));
        }
        // the sweep, in order
        std::fill(held_sender.begin(), held_sender.end(), 0);
        std::fill(moved_sender.begin(), moved_sender.end(), 0);
        held_nonces.clear();
        for (size_t i = 0; i < n; i++) {
            if (J.verdict[i] != OPEN) continue;
            const uint32_t nonce = xp[i * XT_POINTS + P_NONCE];
            bool hold = held_sender[acc_s[i]] || held_nonces.count(nonce);
            if (!hold) {
                if (J.pool[nonce])
                    J.verdict[i] = ZK_BLOCK_NONCE_USED;
                else if (J.refusal[i])
                    J.verdict[i] = ZK_BLOCK_REFUSED_POINT;
                else if (moved_sender[acc_s[i]] || !R.checked[i])
                    hold = true;   // its balance changed in this sweep: the next round verifies it against the new one
                else if (R.checked[i] == 1)
                    J.verdict[i] = ZK_BLOCK_INVALID_PROOF;
                else {
                    J.verdict[i] = ZK_BLOCK_ACCEPTED;
                    J.pool[nonce] = 1;
                    moved_sender[acc_s[i]] = 1;
                    for (uint32_t j = first_sub[i]; j < first_sub[i] + 3; j++) {
                        L.flagv[j] &= ~LEDGER_SKIP;
                        if (!P.on_host) continue;
                        const Op& o = L.ops[j];
                        for (int c = 0; c < 2; c++) {
                            zkwit::EPoint& slot = (o.slot & 1 ? H.pen : H.bal)[(o.slot & ~1u) + c];
                            slot = zkwit::ext_add(slot, zkledger::ext_signed(P.hpt[c ? o.right : o.left], (o.flags & LEDGER_SUB) != 0));
                        }
                    }
                }
            }
            if (hold) {
                held_sender[acc_s[i]] = 1;
                held_nonces.insert(nonce);
            } else {
                J.n_open--;
            }
        }
    }
    // ---- 4. the state to store
    std::vector<uint8_t> enc;
    ZK_TRY(stored_state(A, P, L, J, H, &enc));
    write_accounts(A, P, J, enc.data(), [&](size_t a) { return rolled[a] ? ZK_BLOCK_ROLLED : 0; });
    write_verdicts(A, P, &J);
    return ZK_OK;
}

// zk_g_epoch: GEpoch::group_hash (core/primitives/src/g_epoch.rs:102-110) = find_group_hash (core/jubjub/src/curve/mod.rs:223-247)
// over the epoch's four little-endian bytes and a counter byte from 0, personalised "zcgepoch": group_hash
// (core/jubjub/src/group_hash.rs:17-46) hashes GH_FIRST_BLOCK | tag with BLAKE2s, reads the digest as a point, clears the
// cofactor with three doublings and refuses the identity.
inline zk_status g_epoch(uint32_t epoch, uint8_t out[32]) {
    static const char first_block[65] = "096b36a5804bfacef1691e173c366a47ff5ba84a44f26ddd7e8d9f79d5b42df0";   // core/jubjub/src/constants.rs:5-6
    static const uint8_t person[8] = {'z', 'c', 'g', 'e', 'p', 'o', 'c', 'h'};
    for (uint32_t counter = 0; counter < 255; counter++) {   // (the reference asserts the counter never reaches 255)
        const uint8_t tag[5] = {(uint8_t)epoch, (uint8_t)(epoch >> 8), (uint8_t)(epoch >> 16), (uint8_t)(epoch >> 24), (uint8_t)counter};
        zkhash::Blake2s h(person);
        h.update(first_block, 64);
        h.update(tag, 5);
        uint8_t digest[32];
        h.finish(digest);
        uint64_t v[4];
        zkrt::load_scalar_le(digest, v);
        v[3] &= 0x7fffffffffffffffull;
        zkwit::JPoint p;
        if (zkhost::Fr::geq_p(v) || !zkwit::decode_point(digest, &p)) continue;
        zkwit::EPoint q = zkwit::to_ext(p);
        for (int k = 0; k < 3; k++) q = zkwit::ext_add(q, q);
        if (q.X.is_zero() && q.Y == q.Z) continue;
        zkwit::JPoint aff;
        zkwit::batch_to_affine(&q, &aff, 1);
        zkledger::point_write(aff, out);
        return ZK_OK;
    }
    return fail(ZK_ERR_UNEXPECTED_IDENTITY, "no group hash for epoch " + std::to_string(epoch));
}

}  // namespace zkblock
