// The frame of the three block executors (block_exec.h, anon_block_exec.h, asset_block_exec.h): what a block of extrinsics
// executed in one call needs whatever the module, as plain structs and free functions that each executor calls in its own order.
//   BlockArgs   the arguments the three entries share; null_args, accounts_by_key, check_messages, empty_block
//   Decoded     every DISTINCT 32-byte encoding of the call, keyed by its bytes (Keys32), through ONE k_into_xy launch - or, up
//               to ZKAMD_INTO_XY_HOST_MAX of them (zkxt::into_xy_host_max, read per call), on the host threads: the statuses, the
//               host form's points, acc_bad and the refusal byte of a field table.  An executor puts its extrinsics' encodings,
//               collect_accounts adds four per account and g_epoch, decode starts the decoder.
//   Layout      the ledger as ledger.h's kernels read it: slots (two per account: 2a the balance, 2a + 1 the pending transfer)
//               and ops that point at decoded coordinates BY INDEX, their grouping by slot, the skip bits (flagv: the only
//               thing a verdict moves) and the segments of the work buffer, each starting on 16 bytes.  The constructor carves
//               the common segments; an executor takes its own from cv before to_device, which uploads
//               src | off | perm | pos | slotv | list in one copy, lays the decoded points out with k_block_gather and queues the
//               copy of the statuses.  All of this runs while the decoder is in flight.
//   Judgement   check_signatures (the RedJubjub step, whose hashing runs beside the decoder and whose kernels queue behind the
//               gather; the call's first hipStreamSynchronize follows it), the verdicts, mark_pool, write_accounts, write_verdicts
//   Rows        one verification batch: begin_rows (proofs copied, the rows' buffer: the device form's come back into
//               page-locked memory), the field table in vsrc - written once, for the refusal byte, the host's rows and the
//               device's gather alike - then host_rows or device_rows, and verify_rows.  The buffers live across rounds.
//   HostAccounts, stored_state   the host form's balances and pending transfers in extended coordinates and the encoding of the
//               accounts to store - on the device one more scan under the final skip bits and k_ledger_encode.
// What a module adds is in its own header: its kernels, the ops an extrinsic lays out, its sweep.
// Only verify.cpp includes these headers (they need xt_inputs.h, and the library carries ONE copy of every kernel).
// The data is public chain state: nothing here is constant-time, and the buffers are freed without the wipe.
#pragma once
#include <string>
#include "ledger.h"

namespace zkblock {

using zkdev::Fr;
using zkledger::LEDGER_SCAN_W;
using zkledger::LEDGER_SKIP;
using zkledger::LEDGER_SUB;
using zkrt::fail;
using zkxt::EP;

constexpr uint32_t NO_POINT = 0xffffffffu;

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

// ---- the arguments
struct BlockArgs {
    int device;
    zkxt::IntoXyBufs* xybufs;
    zkrt::DevBuf* work;   // the ledger layout, the scan's results, the rows
    zkrt::PinBuf* pin;    // the rows on their way back
    size_t n;
    const uint8_t *sigs, *msgs;
    const uint64_t* msg_offsets;
    size_t n_acc;
    const zk_block_account* accounts;
    size_t n_pool;
    const uint8_t *nonce_pool, *g_epoch;
    zk_block_account* accounts_out;
    zk_block_verdict* verdicts_out;
    zk_block_stats* stats_out;
};

inline bool null_args(const BlockArgs& A, const void* xts) {
    return (A.n && (!xts || !A.verdicts_out || !A.g_epoch)) || (A.n_acc && (!A.accounts || !A.accounts_out)) || (A.n_pool && !A.nonce_pool) ||
           (A.n && A.sigs && !A.msg_offsets);
}

// the accounts by key: the index of a key is that of its account
inline zk_status accounts_by_key(const BlockArgs& A, Keys32* acc_of) {
    for (size_t a = 0; a < A.n_acc; a++) {
        bool fresh;
        acc_of->put(A.accounts[a].enc_key, &fresh);
        if (!fresh) return fail(ZK_ERR_INVALID_ARGUMENT, "account " + std::to_string(a) + ": its key is that of an earlier account");
    }
    return ZK_OK;
}

// (as redjubjub.h's check_offsets: before anything is launched)
inline zk_status check_messages(const BlockArgs& A) {
    for (size_t i = 0; A.sigs && i < A.n; i++) {
        if (A.msg_offsets[i + 1] < A.msg_offsets[i]) return fail(ZK_ERR_INVALID_ARGUMENT, "msg_offsets decrease at " + std::to_string(i));
        if (A.msg_offsets[i + 1] > A.msg_offsets[i] && !A.msgs)
            return fail(ZK_ERR_INVALID_ARGUMENT, "msgs is null but message " + std::to_string(i) + " is not empty");
    }
    return ZK_OK;
}

// n == 0: the accounts as they came
inline void empty_block(const BlockArgs& A) {
    if (A.n_acc) memcpy(A.accounts_out, A.accounts, A.n_acc * sizeof(zk_block_account));
    if (A.stats_out) *A.stats_out = zk_block_stats{0, 0, 0, 0};
}

// ---- the distinct encodings
struct Decoded {
    Keys32 D;
    std::vector<uint32_t> ap, st;     // ap: four per account - balance left, right, pending left, right; st: the statuses
    uint32_t ge = 0;                  // g_epoch
    size_t nd = 0;
    bool on_host = false;
    std::vector<zkwit::JPoint> hpt;   // host form: the decoded points
    const uint32_t *d_xy = nullptr, *d_st = nullptr;   // device form: k_into_xy's output
    explicit Decoded(size_t expected) : D(expected) {}
};
// after the extrinsics' own encodings: the accounts', g_epoch, and which form the call takes
inline void collect_accounts(const BlockArgs& A, Decoded* P) {
    P->ap.resize(A.n_acc * 4);
    for (size_t a = 0; a < A.n_acc; a++)
        for (int k = 0; k < 2; k++) {
            P->ap[a * 4 + k] = P->D.put(A.accounts[a].balance + 32 * k);
            P->ap[a * 4 + 2 + k] = P->D.put(A.accounts[a].pending + 32 * k);
        }
    P->ge = P->D.put(A.g_epoch);
    P->nd = P->D.size();
    P->on_host = P->nd <= zkxt::into_xy_host_max();
}
// out_extra: bytes the executor keeps behind the statuses in the decoder's output
inline zk_status decode(const BlockArgs& A, Decoded* P, size_t out_extra) {
    ZK_TRY(zkrt::use_device(A.device));
    P->st.resize(P->nd);
    if (P->on_host) {
        P->hpt.resize(P->nd);
        zkxt::into_xy_points(P->nd, [&](size_t p) { return &P->D.enc[p * 32]; }, P->st.data(), P->hpt.data());
        return ZK_OK;
    }
    ZK_TRY(zkxt::into_xy_on_device(P->D.enc.data(), P->nd, A.xybufs, 0, out_extra));
    P->d_xy = A.xybufs->out.as<const uint32_t>();
    P->d_st = P->d_xy + P->nd * 16;
    return ZK_OK;
}
// (the statuses are there once check_signatures has returned)
inline bool acc_bad(const Decoded& P, uint32_t a) { return (P.st[P.ap[a * 4]] | P.st[P.ap[a * 4 + 1]] | P.st[P.ap[a * 4 + 2]] | P.st[P.ap[a * 4 + 3]]) != 0; }
// the refusal byte of a row's field table: (the first refused field + 1) | its status << 6; NO_POINT: a balance, judged with its account
inline uint8_t refusal_of(const Decoded& P, const uint32_t* field, uint32_t n_fields) {
    for (uint32_t k = 0; k < n_fields; k++)
        if (field[k] != NO_POINT && P.st[field[k]]) return (uint8_t)((k + 1) | (P.st[field[k]] << 6));
    return 0;
}

// ---- the ledger layout
struct Layout {
    std::vector<Op> ops;
    std::vector<uint32_t> flagv;
    size_t n_slots, n_ops, np, n_blocks;
    zkledger::Grouping g;
    Carve cv;
    size_t w_lxy, w_lst, w_src, w_off, w_perm, w_pos, w_slotv, w_list, w_flagv, w_cstart, w_pre, w_tot, w_agg, w_carry, w_enc, w_vsrc, w_opv, w_inputs;
    uint32_t* dw = nullptr;   // device form: the work buffer
    zkledger::ScanBufs B{};
    // row_fields: the fields of an input row; list_words: ops whose met values the encoder writes as well (assets)
    Layout(const BlockArgs& A, std::vector<Op>&& ops_, uint32_t row_fields, size_t list_words = 0)
        : ops(std::move(ops_)), flagv(ops.size()), n_slots(2 * A.n_acc), n_ops(ops.size()), np(2 * (n_slots + n_ops)),
          n_blocks((n_ops + LEDGER_SCAN_W - 1) / LEDGER_SCAN_W), g(n_slots, n_ops, [this](size_t j) { return ops[j].slot; }) {
        for (size_t j = 0; j < n_ops; j++) flagv[j] = ops[j].flags;
        w_lxy = cv.take(np * 16), w_lst = cv.take(np);
        w_src = cv.take(np), w_off = cv.take(n_slots + 1), w_perm = cv.take(n_ops), w_pos = cv.take(n_ops), w_slotv = cv.take(n_ops), w_list = cv.take(list_words);
        w_flagv = cv.take(n_ops), w_cstart = cv.take(n_blocks);
        w_pre = cv.take(2 * n_ops * 32), w_tot = cv.take(2 * n_slots * 32), w_agg = cv.take(2 * n_blocks * 32), w_carry = cv.take(2 * n_blocks * 32);
        w_enc = cv.take(2 * (n_slots + list_words) * 8);
        w_vsrc = cv.take(A.n * row_fields), w_opv = cv.take(A.n), w_inputs = cv.take(A.n * row_fields * 16);
    }
    void skip_pair(uint32_t j) { flagv[j] |= LEDGER_SKIP, flagv[j + 1] |= LEDGER_SKIP; }
};

// The rollover of account a where it is due and not yet laid out - at the first extrinsic that names it: the stored pending
// transfer added to the balance and subtracted from the pending slot.  roll_op[a]: the first of the two ops.
inline void push_rollover(const BlockArgs& A, const Decoded& P, uint32_t a, std::vector<uint32_t>* roll_op, std::vector<Op>* ops) {
    if (!(A.accounts[a].flags & ZK_BLOCK_ROLLOVER_DUE) || (*roll_op)[a] != NO_POINT) return;
    (*roll_op)[a] = (uint32_t)ops->size();
    ops->push_back(Op{2 * a, 0, P.ap[a * 4 + 2], P.ap[a * 4 + 3]});
    ops->push_back(Op{2 * a + 1, LEDGER_SUB, P.ap[a * 4 + 2], P.ap[a * 4 + 3]});
}

// The device form: the work buffer, one upload, the first gather, the statuses on their way back.  list: L.w_list's words.
inline zk_status to_device(const BlockArgs& A, Decoded* P, Layout* L, const std::vector<uint32_t>& list = {}) {
    if (P->on_host) return ZK_OK;
    ZK_TRY(A.work->ensure(L->cv.words * 4));
    uint32_t* dw = L->dw = A.work->as<uint32_t>();
    L->B = zkledger::ScanBufs{dw + L->w_lxy,  dw + L->w_lst,    dw + L->w_off, dw + L->w_perm, dw + L->w_pos, dw + L->w_slotv,  dw + L->w_flagv,
                              dw + L->w_cstart, dw + L->w_pre,  dw + L->w_tot, dw + L->w_agg,  dw + L->w_carry, (uint32_t)L->n_slots,
                              (uint32_t)L->n_ops, (uint32_t)L->n_blocks};
    // src | off | perm | pos | slotv | list lie side by side: one upload
    std::vector<uint32_t> up(L->w_flagv - L->w_src, 0);
    std::copy(P->ap.begin(), P->ap.end(), up.begin());
    for (size_t j = 0; j < L->n_ops; j++) {
        up[2 * (L->n_slots + j)] = L->ops[j].left;
        up[2 * (L->n_slots + j) + 1] = L->ops[j].right;
        up[L->w_slotv - L->w_src + j] = L->ops[j].slot;
    }
    std::copy(L->g.off.begin(), L->g.off.end(), up.begin() + (L->w_off - L->w_src));
    std::copy(L->g.perm.begin(), L->g.perm.end(), up.begin() + (L->w_perm - L->w_src));
    std::copy(L->g.pos.begin(), L->g.pos.end(), up.begin() + (L->w_pos - L->w_src));
    std::copy(list.begin(), list.end(), up.begin() + (L->w_list - L->w_src));
    HIP_TRY(hipMemcpyAsync(dw + L->w_src, up.data(), up.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    if (L->n_blocks) HIP_TRY(hipMemcpyAsync(dw + L->w_cstart, L->g.cstart.data(), L->n_blocks * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    if (L->np) {   // (a block of issues alone may come without an account)
        zkrt::ProfScope ps("block_gather");
        ZK_LAUNCH(k_block_gather, dim3((unsigned)((L->np + 255) / 256)), dim3(256), 0, zkrt::g_stream, P->d_xy, P->d_st, (const uint32_t*)(dw + L->w_src),
                  (uint32_t)L->np, dw + L->w_lxy, dw + L->w_lst);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(P->st.data(), P->d_st, P->nd * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
    return ZK_OK;
}
// the skip bits as they stand, ahead of a scan
inline zk_status upload_flags(const Layout& L) {
    if (L.n_blocks) HIP_TRY(hipMemcpyAsync(L.dw + L.w_flagv, L.flagv.data(), L.n_ops * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    return ZK_OK;
}

// ---- the verdicts
enum { OPEN = 255 };
struct Judgement {
    std::vector<uint8_t> sig_ok, sig_why, verdict, refusal, named, pool;   // named: accounts, by a dispatched extrinsic; pool: by decoded point
    size_t n_open = 0;
    zk_block_stats stats = {0, 0, 0, 0};
    explicit Judgement(const BlockArgs& A) : sig_ok(A.n, 1), sig_why(A.n, 0), verdict(A.n, OPEN), refusal(A.n, 0), named(A.n_acc, 0) {}
};
// step 1 of every extrinsic, and the first wait for the stream: the statuses of the decoded points are there afterwards
template <class Xt>
inline zk_status check_signatures(const BlockArgs& A, const Xt* xts, bool on_host, Judgement* J) {
    if (A.sigs) {
        std::vector<uint8_t> vks(A.n * 32);
        for (size_t i = 0; i < A.n; i++) memcpy(&vks[i * 32], xts[i].rvk, 32);
        ZK_TRY(zk_redjubjub_verify_batch(A.n, vks.data(), A.sigs, A.msgs, A.msg_offsets, A.device, J->sig_ok.data(), J->sig_why.data()));
        ZK_TRY(zkrt::use_device(A.device));
    }
    if (!on_host) HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    return ZK_OK;
}
// a nonce of the caller's pool that no extrinsic carries plays no part
inline void mark_pool(const BlockArgs& A, const Decoded& P, Judgement* J) {
    J->pool.assign(P.nd, 0);
    for (size_t k = 0; k < A.n_pool; k++) {
        const uint32_t p = P.D.find(A.nonce_pool + 32 * k);
        if (p != NO_POINT) J->pool[p] = 1;
    }
}
// enc: 64 bytes per slot.  flags_of(a): what a named account's flags gain.
template <class FlagsOf>
inline void write_accounts(const BlockArgs& A, const Decoded& P, const Judgement& J, const uint8_t* enc, FlagsOf&& flags_of) {
    for (size_t a = 0; a < A.n_acc; a++) {
        zk_block_account out = A.accounts[a];
        if (J.named[a]) {
            if (acc_bad(P, (uint32_t)a)) {
                memset(out.balance, 0, 64);
                memset(out.pending, 0, 64);
            } else {
                memcpy(out.balance, &enc[(2 * a) * 64], 64);
                memcpy(out.pending, &enc[(2 * a + 1) * 64], 64);
            }
            out.flags |= flags_of(a);
        }
        A.accounts_out[a] = out;
    }
}
inline void write_verdicts(const BlockArgs& A, const Decoded& P, Judgement* J) {
    for (size_t i = 0; i < A.n; i++) {
        const uint8_t v = J->verdict[i];
        A.verdicts_out[i] = zk_block_verdict{v, (uint8_t)(v == ZK_BLOCK_BAD_SIGNATURE ? J->sig_why[i] : v == ZK_BLOCK_REFUSED_POINT ? J->refusal[i] : 0), 0};
    }
    J->stats.points_decoded = (uint32_t)P.nd;
    if (A.stats_out) *A.stats_out = J->stats;
}

// ---- one verification batch
struct Rows {
    uint32_t fields;   // of a row: 64 bytes each, x then y, plain little-endian
    std::vector<uint32_t> todo, vsrc, opv;   // the extrinsics of the batch; the rows' field table; the op whose slot's value a row meets
    std::vector<uint8_t> proofs, inputs, ok, checked;   // checked: by extrinsic - 0 not in a batch, 1 rejected, 2 verified
    uint8_t* in_rows = nullptr;
};
// for the extrinsics in R->todo
template <class Xt>
inline zk_status begin_rows(const BlockArgs& A, const Decoded& P, const Xt* xts, Rows* R) {
    const size_t nv = R->todo.size();
    R->proofs.resize(nv * 192);
    for (size_t v = 0; v < nv; v++) memcpy(&R->proofs[v * 192], xts[R->todo[v]].proof, 192);
    if (P.on_host) {
        R->inputs.assign(nv * R->fields * 64, 0);
        R->in_rows = R->inputs.data();
    } else {   // the device form's rows come back into page-locked memory, copied at the link's rate
        ZK_TRY(A.pin->ensure(nv * R->fields * 64));
        R->in_rows = A.pin->as<uint8_t>();
    }
    R->ok.assign(nv, 0);
    R->vsrc.resize(nv * R->fields);
    R->opv.resize(nv);
    return ZK_OK;
}
// the host form's rows from the field table; a NO_POINT at field 7 or 8 of row v is met[2 v], met[2 v + 1]
inline void host_rows(const Decoded& P, const zkwit::JPoint* met, Rows* R) {
    for (size_t f = 0; f < R->vsrc.size(); f++) {
        const zkwit::JPoint& q = R->vsrc[f] == NO_POINT ? met[2 * (f / R->fields) + (f % R->fields - 6)] : P.hpt[R->vsrc[f]];
        const zkhost::Fr x = q.x.from_mont(), y = q.y.from_mont();
        memcpy(R->in_rows + f * 64, x.l, 32);
        memcpy(R->in_rows + f * 64 + 32, y.l, 32);
    }
}
inline void gather_rows(const Decoded& P, const Layout& L, const Rows& R) {
    zkrt::ProfScope ps("block_gather");
    ZK_LAUNCH(k_block_gather, dim3((unsigned)((R.vsrc.size() + 255) / 256)), dim3(256), 0, zkrt::g_stream, P.d_xy, P.d_st, (const uint32_t*)(L.dw + L.w_vsrc),
              (uint32_t)R.vsrc.size(), L.dw + L.w_inputs, (uint32_t*)nullptr);
}
inline zk_status fetch_rows(const Layout& L, const Rows& R) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R.in_rows, L.dw + L.w_inputs, R.vsrc.size() * 64, hipMemcpyDeviceToHost, zkrt::g_stream));
    HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    return ZK_OK;
}
// the device form's rows: the field table gathered, then balance(), the kernel that fills fields 7 and 8 from the scan
template <class Balance>
inline zk_status device_rows(const Decoded& P, const Layout& L, const Rows& R, Balance&& balance) {
    HIP_TRY(hipMemcpyAsync(L.dw + L.w_vsrc, R.vsrc.data(), R.vsrc.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    HIP_TRY(hipMemcpyAsync(L.dw + L.w_opv, R.opv.data(), R.opv.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
    gather_rows(P, L, R);
    balance();
    return fetch_rows(L, R);
}
template <class Verify>
inline zk_status verify_rows(const BlockArgs& A, Verify&& verify, Rows* R, Judgement* J) {
    const size_t nv = R->todo.size();
    ZK_TRY(verify(nv, R->proofs.data(), R->in_rows, R->ok.data()));
    ZK_TRY(zkrt::use_device(A.device));
    J->stats.proofs_verified += (uint32_t)nv;
    for (size_t v = 0; v < nv; v++) R->checked[R->todo[v]] = (uint8_t)(1 + R->ok[v]);
    return ZK_OK;
}

// ---- the host form's state: every named, readable account, rolled over where that happens
struct HostAccounts {
    std::vector<zkwit::EPoint> bal, pen;   // 2 a + c
};
inline void host_accounts(const BlockArgs& A, const Decoded& P, const Judgement& J, const std::vector<uint8_t>& rolled, HostAccounts* H) {
    if (!P.on_host) return;
    H->bal.resize(2 * A.n_acc);
    H->pen.resize(2 * A.n_acc);
    for (size_t a = 0; a < A.n_acc; a++) {
        if (!J.named[a] || acc_bad(P, (uint32_t)a)) continue;
        for (int c = 0; c < 2; c++) {
            H->bal[2 * a + c] = zkwit::to_ext(P.hpt[P.ap[a * 4 + c]]);
            H->pen[2 * a + c] = zkwit::to_ext(P.hpt[P.ap[a * 4 + 2 + c]]);
            if (rolled[a]) {
                H->bal[2 * a + c] = zkwit::ext_add(H->bal[2 * a + c], H->pen[2 * a + c]);
                H->pen[2 * a + c] = zkwit::ext_zero();
            }
        }
    }
}
// the accounts to store, 64 bytes per slot: the host's state made affine, or one more scan under the final skip bits and
// k_ledger_encode over the slot outputs
inline zk_status stored_state(const BlockArgs& A, const Decoded& P, const Layout& L, const Judgement& J, const HostAccounts& H, std::vector<uint8_t>* enc) {
    enc->assign(L.n_slots * 64, 0);
    if (P.on_host) {
        std::vector<zkwit::EPoint> vals;
        std::vector<uint8_t*> to;
        for (size_t a = 0; a < A.n_acc; a++) {
            if (!J.named[a] || acc_bad(P, (uint32_t)a)) continue;
            for (int c = 0; c < 2; c++) {
                vals.push_back(H.bal[2 * a + c]);
                to.push_back(&(*enc)[(2 * a) * 64 + 32 * c]);
                vals.push_back(H.pen[2 * a + c]);
                to.push_back(&(*enc)[(2 * a + 1) * 64 + 32 * c]);
            }
        }
        std::vector<zkwit::JPoint> aff(vals.size());
        zkwit::batch_to_affine(vals.data(), aff.data(), vals.size());
        for (size_t k = 0; k < aff.size(); k++) zkledger::point_write(aff[k], to[k]);
        return ZK_OK;
    }
    ZK_TRY(upload_flags(L));
    zkledger::launch_scan(L.B);
    zkledger::launch_encode(L.B, 2 * L.n_slots, L.dw + L.w_enc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(enc->data(), L.dw + L.w_enc, L.n_slots * 64, hipMemcpyDeviceToHost, zkrt::g_stream));
    HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
    return ZK_OK;
}

}  // namespace zkblock
