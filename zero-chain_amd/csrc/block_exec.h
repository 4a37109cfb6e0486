// A block of confidential transfers executed in one call (zk_confidential_block_execute): what
//   encrypted_balances::confidential_transfer (modules/encrypted-balances/src/lib.rs:25-96) does to storage for every extrinsic
//   of a block in order - ensure_signed, rollover of sender and recipient (:133-170), the nonce pool (:49, :69),
//   verify_confidential_proof against the sender's balance AS IT STANDS (modules/zk-system/src/lib.rs:56-115), sub_enc_balance
//   and add_pending_transfer (:173-222) - with the reference's verdict for every extrinsic and the state to store.
// The parts are the library's own: k_into_xy (xt_inputs.h), the segmented scan of ledger.h, zkrt::verify_batch, the RedJubjub
// check.  What this header adds is the join:
//   1. Every DISTINCT 32-byte encoding of the call - eight per extrinsic (both keys, the three lefts, the randomness, rvk,
//      nonce), four per account (balance and pending, left and right), g_epoch - goes through ONE k_into_xy launch, keyed by
//      its bytes.  A key, a g_epoch or a randomness that recurs is decoded once.
//   2. The ledger's slots (two per account: 2a the balance, 2a + 1 the pending transfer) and ops (rollover: the stored pending
//      added to the balance and subtracted from the pending slot; two subtractions; one addition - INTEGRATION.md 8.13) point
//      at decoded coordinates BY INDEX.  k_block_gather lays the decoded points out as k_ledger_scan / k_ledger_carry /
//      k_ledger_encode read them, so those three run unchanged and zk_elgamal_ledger_apply keeps its bytes.
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
//   5. The inputs of a round cross the host once (704 bytes per extrinsic) into zkrt::verify_batch, which stages its own uploads.
//   6. After the last round one more scan with the final skip bits, and k_ledger_encode over the 2 x 2 x n_accounts slot
//      outputs only, gives the accounts to store.
// Two forms, the same bytes: up to ZKAMD_INTO_XY_HOST_MAX distinct points (read per call, as ledger.h) the point work - decode,
// balances, encode - runs on the host threads; the verification always runs on the key's device.
// Only verify.cpp includes this header (it needs xt_inputs.h, and the library carries ONE k_into_xy).
// The data is public chain state: nothing here is constant-time, and the buffers are freed without the wipe.
#pragma once
#include <string>
#include <unordered_set>
#include "ledger.h"

namespace zkblock {

using zkdev::Fr;
using zkledger::LEDGER_SCAN_W;
using zkledger::LEDGER_SKIP;
using zkledger::LEDGER_SUB;
using zkrt::fail;
using zkxt::EP;

constexpr uint32_t NO_POINT = 0xffffffffu;
constexpr uint32_t XT_POINTS = 8, XT_FIELDS = 11, XT_INPUT_WORDS = 2 * XT_FIELDS * 8;
// the eight encodings of an extrinsic in the order they are collected, and the field of zk_confidential_verify_batch each is
enum { P_SENDER = 0, P_RECIPIENT, P_AMOUNT_SENDER, P_AMOUNT_RECIPIENT, P_RANDOMNESS, P_FEE, P_RVK, P_NONCE };

// ---- device side
// out[j] = the decoded point src[j] (16 coordinate words; its status where st_out is given); NO_POINT leaves the place alone
static __global__ void __launch_bounds__(256)
k_block_gather(const uint32_t* xy, const uint32_t* st, const uint32_t* src, uint32_t n, uint32_t* xy_out, uint32_t* st_out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = src[j];
    if (s == NO_POINT) return;
    const uint4* in = reinterpret_cast<const uint4*>(xy + (size_t)s * 16);
    uint4* out = reinterpret_cast<uint4*>(xy_out + (size_t)j * 16);
    out[0] = in[0];
    out[1] = in[1];
    out[2] = in[2];
    out[3] = in[3];
    if (st_out) st_out[j] = st[s];
}

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
        const Fr d2 = zkledger::edwards_2d();
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

// ---- host side
struct Op {
    uint32_t slot, flags, left, right;   // left, right: indices of decoded points
};

// 32-byte keys in order of arrival, found again by their bytes: open addressing over a hash of all 32 bytes, no allocation per
// key (a block of 4096 transfers has 45 057 of them, and the decoder cannot start before they are collected)
struct Keys32 {
    std::vector<uint32_t> cell;   // index + 1; 0 = empty
    std::vector<uint8_t> enc;
    size_t mask;
    explicit Keys32(size_t expected) {
        size_t cap = 16;
        while (cap < 2 * expected + 2) cap <<= 1;
        cell.assign(cap, 0);
        mask = cap - 1;
        enc.reserve(expected * 32);
    }
    size_t size() const { return enc.size() / 32; }
    static uint64_t hash(const uint8_t* b) {
        uint64_t w[4];
        memcpy(w, b, 32);
        uint64_t h = w[0] * 0x9e3779b97f4a7c15ull;
        h = ((h ^ (h >> 29)) + w[1]) * 0xbf58476d1ce4e5b9ull;
        h = ((h ^ (h >> 31)) + w[2]) * 0x94d049bb133111ebull;
        h = ((h ^ (h >> 30)) + w[3]) * 0x9e3779b97f4a7c15ull;
        return h ^ (h >> 32);
    }
    uint32_t find(const uint8_t* b) const {   // NO_POINT where absent
        for (size_t at = hash(b) & mask;; at = (at + 1) & mask) {
            const uint32_t c = cell[at];
            if (!c) return NO_POINT;
            if (!memcmp(&enc[(size_t)(c - 1) * 32], b, 32)) return c - 1;
        }
    }
    uint32_t put(const uint8_t* b, bool* fresh = nullptr) {
        for (size_t at = hash(b) & mask;; at = (at + 1) & mask) {
            const uint32_t c = cell[at];
            if (c && !memcmp(&enc[(size_t)(c - 1) * 32], b, 32)) {
                if (fresh) *fresh = false;
                return c - 1;
            }
            if (!c) {
                enc.insert(enc.end(), b, b + 32);
                cell[at] = (uint32_t)size();
                if (fresh) *fresh = true;
                return cell[at] - 1;
            }
        }
    }
};

// segments of one device buffer, each starting on 16 bytes
struct Carve {
    size_t words = 0;
    size_t take(size_t n) {
        const size_t at = words;
        words += (n + 3) / 4 * 4;
        return at;
    }
};

// verify(n_v, proofs, inputs, ok): zkrt::verify_batch on the key (verify.cpp hands it in: zk_vk is defined there)
template <class Verify>
inline zk_status execute(int device, zkxt::IntoXyBufs* xybufs, zkrt::DevBuf* work, zkrt::PinBuf* pin, Verify&& verify, size_t n, const zk_confidential_xt* xts,
                         const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n_acc, const zk_block_account* accounts,
                         size_t n_pool, const uint8_t* nonce_pool, const uint8_t* g_epoch, zk_block_account* accounts_out,
                         zk_block_verdict* verdicts_out, zk_block_stats* stats_out) {
    if ((n && (!xts || !verdicts_out || !g_epoch)) || (n_acc && (!accounts || !accounts_out)) || (n_pool && !nonce_pool) ||
        (n && sigs && !msg_offsets))
        return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (size_t)1 << 24 || n_acc > (size_t)1 << 24) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^24 extrinsics or accounts in one call");
    // ---- the accounts by key, the extrinsics' accounts
    Keys32 acc_of(n_acc);   // (the index of a key is that of its account)
    for (size_t a = 0; a < n_acc; a++) {
        bool fresh;
        acc_of.put(accounts[a].enc_key, &fresh);
        if (!fresh) return fail(ZK_ERR_INVALID_ARGUMENT, "account " + std::to_string(a) + ": its key is that of an earlier account");
    }
    std::vector<uint32_t> acc_s(n), acc_r(n);
    for (size_t i = 0; i < n; i++) {
        acc_s[i] = acc_of.find(xts[i].enc_key_sender);
        acc_r[i] = acc_of.find(xts[i].enc_key_recipient);
        if (acc_s[i] == NO_POINT) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the sender's key is not among the accounts");
        if (acc_r[i] == NO_POINT) return fail(ZK_ERR_INVALID_ARGUMENT, "extrinsic " + std::to_string(i) + ": the recipient's key is not among the accounts");
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
    Keys32 D(n * XT_POINTS + n_acc * 4 + 1);
    std::vector<uint32_t> xp(n * XT_POINTS), ap(n_acc * 4);
    for (size_t i = 0; i < n; i++) {
        const zk_confidential_xt& x = xts[i];
        const uint8_t* f[XT_POINTS] = {x.enc_key_sender, x.enc_key_recipient, x.left_amount_sender, x.left_amount_recipient,
                                       x.right_randomness, x.left_fee, x.rvk, x.nonce};
        for (uint32_t k = 0; k < XT_POINTS; k++) xp[i * XT_POINTS + k] = D.put(f[k]);
    }
    for (size_t a = 0; a < n_acc; a++) {
        for (int k = 0; k < 2; k++) {
            ap[a * 4 + k] = D.put(accounts[a].balance + 32 * k);
            ap[a * 4 + 2 + k] = D.put(accounts[a].pending + 32 * k);
        }
    }
    const uint32_t ge = D.put(g_epoch);
    const size_t nd = D.size();
    stats.points_decoded = (uint32_t)nd;
    const char* e = getenv("ZKAMD_INTO_XY_HOST_MAX");
    const size_t host_max = e && *e ? (size_t)strtoull(e, nullptr, 10) : zkxt::INTO_XY_HOST_MAX;
    const bool on_host = nd <= host_max;
    ZK_TRY(zkrt::use_device(device));
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
        ZK_TRY(zkxt::into_xy_on_device(D.enc.data(), nd, xybufs, 0, 0));
    }
    // ---- 2. slots and ops, while the decoder runs.  Every extrinsic gets its three ops, and the first one to name a due account
    // carries that account's rollover: the order of the ops does not depend on any verdict, only their skip bits do.  Whether a
    // rollover happens is known once the signatures and the stored ciphertexts are judged.
    const size_t n_slots = 2 * n_acc;
    std::vector<Op> ops;
    ops.reserve(4 * n + 2 * n_acc);
    std::vector<uint32_t> first_sub(n), roll_op(n_acc, NO_POINT);   // roll_op: the first of the account's two rollover ops
    for (size_t i = 0; i < n; i++) {
        const uint32_t two[2] = {acc_s[i], acc_r[i]};
        for (int k = 0; k < 2; k++) {
            const uint32_t a = two[k];
            if (!(accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) || roll_op[a] != NO_POINT) continue;
            roll_op[a] = (uint32_t)ops.size();
            ops.push_back(Op{2 * a, 0, ap[a * 4 + 2], ap[a * 4 + 3]});
            ops.push_back(Op{2 * a + 1, LEDGER_SUB, ap[a * 4 + 2], ap[a * 4 + 3]});
        }
        const uint32_t* p = &xp[i * XT_POINTS];
        first_sub[i] = (uint32_t)ops.size();
        ops.push_back(Op{2 * acc_s[i], LEDGER_SUB | LEDGER_SKIP, p[P_AMOUNT_SENDER], p[P_RANDOMNESS]});
        ops.push_back(Op{2 * acc_s[i], LEDGER_SUB | LEDGER_SKIP, p[P_FEE], p[P_RANDOMNESS]});
        ops.push_back(Op{2 * acc_r[i] + 1, LEDGER_SKIP, p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS]});
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
                 w_carry = cv.take(2 * n_blocks * 32), w_enc = cv.take(2 * n_slots * 8), w_vsrc = cv.take(n * XT_FIELDS), w_opv = cv.take(n),
                 w_inputs = cv.take(n * XT_INPUT_WORDS);
    uint32_t* dw = nullptr;
    const uint32_t *d_xy = nullptr, *d_st = nullptr;
    std::vector<uint32_t> flagv(n_ops);
    for (size_t j = 0; j < n_ops; j++) flagv[j] = ops[j].flags;
    if (!on_host) {
        ZK_TRY(work->ensure(cv.words * 4));
        dw = work->as<uint32_t>();
        d_xy = xybufs->out.as<const uint32_t>();
        d_st = d_xy + nd * 16;
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
    // ---- step 1 of every extrinsic: the signatures (the check's kernels queue behind the decoder and the
    // gather, its hashing runs beside them)
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
        if (sig_ok[i]) named[acc_s[i]] = named[acc_r[i]] = 1;
    // ---- steps 2 and 5 as far as they do not depend on the order: unreadable accounts, refused points
    auto acc_bad = [&](uint32_t a) { return (dst[ap[a * 4]] | dst[ap[a * 4 + 1]] | dst[ap[a * 4 + 2]] | dst[ap[a * 4 + 3]]) != 0; };
    enum { OPEN = 255 };
    std::vector<uint8_t> verdict(n, OPEN), refusal(n, 0);
    std::vector<uint8_t> rolled(n_acc, 0);
    size_t n_open = 0;
    for (size_t i = 0; i < n; i++) {
        if (!sig_ok[i]) {
            verdict[i] = ZK_BLOCK_BAD_SIGNATURE;
            continue;
        }
        if (acc_bad(acc_s[i]) || acc_bad(acc_r[i])) {
            verdict[i] = ZK_BLOCK_BAD_ACCOUNT;
            continue;
        }
        rolled[acc_s[i]] = rolled[acc_r[i]] = 1;   // (of a due account: step 3 is reached)
        const uint32_t* p = &xp[i * XT_POINTS];
        const uint32_t field[XT_FIELDS] = {p[P_SENDER], p[P_RECIPIENT], p[P_AMOUNT_SENDER], p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS], p[P_FEE],
                                           NO_POINT,    NO_POINT,       p[P_RVK],           ge,                    p[P_NONCE]};
        for (uint32_t k = 0; k < XT_FIELDS && !refusal[i]; k++)
            if (field[k] != NO_POINT && dst[field[k]]) refusal[i] = (uint8_t)((k + 1) | (dst[field[k]] << 6));
        n_open++;
    }
    for (size_t a = 0; a < n_acc; a++) {
        rolled[a] = rolled[a] && (accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE);
        if (roll_op[a] != NO_POINT && !rolled[a]) flagv[roll_op[a]] |= LEDGER_SKIP, flagv[roll_op[a] + 1] |= LEDGER_SKIP;
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
    auto ext_of = [&](uint32_t p, bool negative) {
        zkwit::EPoint a = zkwit::to_ext(hpt[p]);
        if (negative) {
            a.X = zkhost::Fr::zero() - a.X;
            a.T = zkhost::Fr::zero() - a.T;
        }
        return a;
    };
    auto scan = [&]() -> zk_status {   // the ledger's scan under the skip bits as they stand
        if (!n_blocks) return ZK_OK;
        HIP_TRY(hipMemcpyAsync(dw + w_flagv, flagv.data(), n_ops * 4, hipMemcpyHostToDevice, zkrt::g_stream));
        zkrt::ProfScope ps("ledger_scan");
        ZK_LAUNCH_SYNC(zkledger::k_ledger_scan, dim3((unsigned)n_blocks, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)(dw + w_lxy),
                       (const uint32_t*)(dw + w_lst), (const uint32_t*)(dw + w_off), (const uint32_t*)(dw + w_perm), (const uint32_t*)(dw + w_slotv),
                       (const uint32_t*)(dw + w_flagv), (uint32_t)n_slots, (uint32_t)n_ops, dw + w_pre, dw + w_tot, dw + w_agg);
        ZK_LAUNCH_SYNC(zkledger::k_ledger_carry, dim3(1, 2), dim3(LEDGER_SCAN_W), 0, zkrt::g_stream, (const uint32_t*)(dw + w_agg),
                       (const uint32_t*)(dw + w_cstart), (uint32_t)n_blocks, dw + w_carry);
        return ZK_OK;
    };
    // ---- 3. the rounds
    std::vector<uint8_t> pool(nd, 0);   // by decoded point: a nonce of the caller's pool that no extrinsic carries plays no part
    for (size_t k = 0; k < n_pool; k++) {
        const uint32_t p = D.find(nonce_pool + 32 * k);
        if (p != NO_POINT) pool[p] = 1;
    }
    std::vector<uint32_t> todo, vsrc, opv;
    std::vector<uint8_t> proofs, inputs, ok, checked(n), held_sender(n_acc), moved_sender(n_acc);
    std::unordered_set<uint32_t> held_nonces;
    while (n_open) {
        stats.rounds++;
        todo.clear();
        for (size_t i = 0; i < n; i++)
            if (verdict[i] == OPEN && !refusal[i] && !pool[xp[i * XT_POINTS + P_NONCE]]) todo.push_back((uint32_t)i);
        const size_t nv = todo.size();
        std::fill(checked.begin(), checked.end(), 0);
        if (nv) {
            proofs.resize(nv * 192);
            uint8_t* in_rows;   // the device form's rows come back into page-locked memory: 704 bytes per extrinsic, copied at the link's rate
            if (on_host) {
                inputs.assign(nv * XT_INPUT_WORDS * 4, 0);
                in_rows = inputs.data();
            } else {
                ZK_TRY(pin->ensure(nv * XT_INPUT_WORDS * 4));
                in_rows = pin->as<uint8_t>();
            }
            ok.assign(nv, 0);
            for (size_t v = 0; v < nv; v++) memcpy(&proofs[v * 192], xts[todo[v]].proof, 192);
            if (on_host) {
                std::vector<zkwit::EPoint> vals(2 * nv);
                for (size_t v = 0; v < nv; v++)
                    for (int c = 0; c < 2; c++) vals[2 * v + c] = hbal[2 * acc_s[todo[v]] + c];
                std::vector<zkwit::JPoint> aff(2 * nv);
                zkwit::batch_to_affine(vals.data(), aff.data(), 2 * nv);
                for (size_t v = 0; v < nv; v++) {
                    const uint32_t i = todo[v], *p = &xp[i * XT_POINTS];
                    const uint32_t field[XT_FIELDS] = {p[P_SENDER], p[P_RECIPIENT], p[P_AMOUNT_SENDER], p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS], p[P_FEE],
                                                       NO_POINT,    NO_POINT,       p[P_RVK],           ge,                    p[P_NONCE]};
                    for (uint32_t k = 0; k < XT_FIELDS; k++) {
                        const zkwit::JPoint& q = field[k] == NO_POINT ? aff[2 * v + (k - 6)] : hpt[field[k]];
                        const zkhost::Fr x = q.x.from_mont(), y = q.y.from_mont();
                        memcpy(in_rows + (v * XT_FIELDS + k) * 64, x.l, 32);
                        memcpy(in_rows + (v * XT_FIELDS + k) * 64 + 32, y.l, 32);
                    }
                }
            } else {
                ZK_TRY(scan());
                vsrc.resize(nv * XT_FIELDS);
                opv.resize(nv);
                for (size_t v = 0; v < nv; v++) {
                    const uint32_t i = todo[v], *p = &xp[i * XT_POINTS];
                    const uint32_t field[XT_FIELDS] = {p[P_SENDER], p[P_RECIPIENT], p[P_AMOUNT_SENDER], p[P_AMOUNT_RECIPIENT], p[P_RANDOMNESS], p[P_FEE],
                                                       NO_POINT,    NO_POINT,       p[P_RVK],           ge,                    p[P_NONCE]};
                    std::copy(field, field + XT_FIELDS, &vsrc[v * XT_FIELDS]);
                    opv[v] = first_sub[i];
                }
                HIP_TRY(hipMemcpyAsync(dw + w_vsrc, vsrc.data(), vsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
                HIP_TRY(hipMemcpyAsync(dw + w_opv, opv.data(), nv * 4, hipMemcpyHostToDevice, zkrt::g_stream));
                {
                    zkrt::ProfScope ps("block_gather");
                    ZK_LAUNCH(k_block_gather, dim3((unsigned)((nv * XT_FIELDS + 255) / 256)), dim3(256), 0, zkrt::g_stream, d_xy, d_st,
                              (const uint32_t*)(dw + w_vsrc), (uint32_t)(nv * XT_FIELDS), dw + w_inputs, (uint32_t*)nullptr);
                }
                {
                    zkrt::ProfScope ps("block_balance_xy");
                    ZK_LAUNCH(k_block_balance_xy, dim3((unsigned)((2 * nv + 63) / 64)), dim3(64), 0, zkrt::g_stream, (const uint32_t*)(dw + w_lxy),
                              (const uint32_t*)(dw + w_lst), (const uint32_t*)(dw + w_off), (const uint32_t*)(dw + w_pos), (const uint32_t*)(dw + w_slotv),
                              (const uint32_t*)(dw + w_pre), (const uint32_t*)(dw + w_carry), (const uint32_t*)(dw + w_opv), (uint32_t)n_ops,
                              (uint32_t)n_blocks, (uint32_t)nv, dw + w_inputs);
                }
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(in_rows, dw + w_inputs, nv * XT_INPUT_WORDS * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
                HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
            }
            ZK_TRY(verify(nv, proofs.data(), in_rows, ok.data()));
            ZK_TRY(zkrt::use_device(device));
            stats.proofs_verified += (uint32_t)nv;
            for (size_t v = 0; v < nv; v++) checked[todo[v]] = (uint8_t)(1 + ok[v]);
        }
        // the sweep, in order
        std::fill(held_sender.begin(), held_sender.end(), 0);
        std::fill(moved_sender.begin(), moved_sender.end(), 0);
        held_nonces.clear();
        for (size_t i = 0; i < n; i++) {
            if (verdict[i] != OPEN) continue;
            const uint32_t nonce = xp[i * XT_POINTS + P_NONCE];
            bool hold = held_sender[acc_s[i]] || held_nonces.count(nonce);
            if (!hold) {
                if (pool[nonce])
                    verdict[i] = ZK_BLOCK_NONCE_USED;
                else if (refusal[i])
                    verdict[i] = ZK_BLOCK_REFUSED_POINT;
                else if (moved_sender[acc_s[i]] || !checked[i])
                    hold = true;   // its balance changed in this sweep: the next round verifies it against the new one
                else if (checked[i] == 1)
                    verdict[i] = ZK_BLOCK_INVALID_PROOF;
                else {
                    verdict[i] = ZK_BLOCK_ACCEPTED;
                    pool[nonce] = 1;
                    moved_sender[acc_s[i]] = 1;
                    for (uint32_t j = first_sub[i]; j < first_sub[i] + 3; j++) {
                        flagv[j] &= ~LEDGER_SKIP;
                        if (!on_host) continue;
                        for (int c = 0; c < 2; c++) {
                            zkwit::EPoint& slot = (ops[j].slot & 1 ? hpen : hbal)[(ops[j].slot & ~1u) + c];
                            slot = zkwit::ext_add(slot, ext_of(c ? ops[j].right : ops[j].left, (ops[j].flags & LEDGER_SUB) != 0));
                        }
                    }
                }
            }
            if (hold) {
                held_sender[acc_s[i]] = 1;
                held_nonces.insert(nonce);
            } else {
                n_open--;
            }
        }
    }
    // ---- 4. the state to store
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
        ZK_TRY(scan());
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
