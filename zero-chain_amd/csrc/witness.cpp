// libzkamd, witness half: the GPU witness generators of the two built-in circuits - the confidential transfer (kernels:
// witness_gpu.h) and the anonymous transfer (witness_anon_gpu.h) - as the statement route (statement_route.h), zk_pipeline and
// gen_proof drive them: one slot prologue and epilogue, each circuit's launches between them, each circuit's finish; and the
// discrete-log search of zk_elgamal_decrypt (kernels: elgamal_dlog.h; its C entries are wallet.cpp's).
#include <algorithm>
#include "handles.h"
#include "transfer_witness.h"
#include "witness_gpu.h"
#include "witness_anon_gpu.h"
#include "elgamal_dlog.h"

using namespace zkrt;

// ---- the same on the GPU (witness_gpu.h): np statements -> R->work.z[slot], enqueued on `stream`
static zk_status witness_gpu_init(zk_r1cs* R) {
    if (R->work.wit_ready) return ZK_OK;
    static_assert(sizeof(zkwitdev::Stmt) == sizeof(zk_transfer_statement), "statement layout");
    const zkwit::Tables& t = zkwit::tables();
    static_assert(sizeof(zkwit::JPoint) == 64, "Jubjub point layout");
    ZK_TRY(R->work.wit_table.ensure(84 * 8 * sizeof(zkwit::JPoint)));
    HIP_TRY(hipMemcpy(R->work.wit_table.p, t.win.data(), 84 * 8 * sizeof(zkwit::JPoint), hipMemcpyHostToDevice));
    const zkhost::Fr dd[2] = {zkwit::edwards_d(), zkwit::edwards_d().dbl()};
    ZK_TRY(R->work.wit_consts.ensure(sizeof(dd)));
    HIP_TRY(hipMemcpy(R->work.wit_consts.p, dd, sizeof(dd), hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++)
        if (!R->work.wit_done[k]) HIP_TRY(hipEventCreate(&R->work.wit_done[k]));
    R->work.wit_ready = true;
    return ZK_OK;
}
// What the witness kernels of a circuit need of a slot beside its statements: variables per statement, bytes of a statement,
// points that travel between the levels, roles of the chain scratch
struct SlotSizes {
    size_t nv, st_size, points, scratch_roles;
};
// The prologue both circuits share, in two steps.  stage: the buffers of the slot, and the np statements copied into its pinned
// half, where the caller may still touch them.  begin: their upload, wit_bad filled with the circuit's "nothing found", and the
// Ctx of the slot, all but its statements.
static zk_status witness_slot_stage(zk_r1cs* R, const SlotSizes& S, const void* st, size_t np, int slot) {
    ZK_TRY(witness_gpu_init(R));
    ZK_TRY(R->work.z[slot].ensure(np * S.nv * 32));
    ZK_TRY(R->work.wit_st[slot].ensure(np * S.st_size));
    ZK_TRY(R->work.wit_bad[slot].ensure(np * 4));
    ZK_TRY(R->work.pin_st[slot].ensure(np * S.st_size));
    ZK_TRY(R->work.pin_bad[slot].ensure(np * 4));
    ZK_TRY(R->work.wit_pts.ensure(np * S.points * 64));
    ZK_TRY(R->work.wit_scratch.ensure(S.scratch_roles * zkwitdev::SCRATCH_SLOTS * np * 32));
    memcpy(R->work.pin_st[slot].p, st, np * S.st_size);
    return ZK_OK;
}
static zk_status witness_slot_begin(zk_r1cs* R, const SlotSizes& S, size_t np, int slot, hipStream_t stream, int bad_fill, zkwitdev::Ctx* c) {
    HIP_TRY(hipMemcpyAsync(R->work.wit_st[slot].p, R->work.pin_st[slot].p, np * S.st_size, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(R->work.wit_bad[slot].p, bad_fill, np * 4, stream));
    c->z = R->work.z[slot].as<uint32_t>();
    c->st = nullptr;
    c->pts = R->work.wit_pts.as<uint32_t>();
    c->table = R->work.wit_table.as<uint32_t>();
    c->consts = R->work.wit_consts.as<uint32_t>();
    c->scratch = R->work.wit_scratch.as<uint32_t>();
    c->bad = R->work.wit_bad[slot].as<uint32_t>();
    c->n = (uint32_t)np;
    return ZK_OK;
}
// ... and the epilogue, behind the circuit's launches: what they found on its way to the pinned half, the event finish() waits for
static zk_status witness_slot_end(zk_r1cs* R, size_t np, int slot, hipStream_t stream) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R->work.pin_bad[slot].p, R->work.wit_bad[slot].p, np * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(R->work.wit_done[slot], stream));
    return ZK_OK;
}

zk_status witness_gpu_enqueue(zk_r1cs* R, const zk_transfer_statement* st, size_t np, int slot, hipStream_t stream, bool typed_inputs) {
    const SlotSizes S = {zkwitdev::NV, sizeof(zkwitdev::Stmt), zkwitdev::P_COUNT, zkwitdev::L1_SCRATCH_ROLES};
    ZK_TRY(witness_slot_stage(R, S, st, np, slot));
    zkwitdev::Ctx c;
    ZK_TRY(witness_slot_begin(R, S, np, slot, stream, 0, &c));
    c.st = R->work.wit_st[slot].as<zkwitdev::Stmt>();
    const unsigned b64 = (unsigned)((np + 63) / 64);
    {
        ProfScope ps("witness_gpu", stream);
        ZK_LAUNCH(zkwitdev::k_wit_decode, dim3((unsigned)((np * 5 + 63) / 64)), dim3(64), 0, stream, c);
        ZK_LAUNCH(zkwitdev::k_wit_level1, dim3(b64, zkwitdev::L1_ROLES + (typed_inputs ? zkwitdev::L1_TYPED_ROLES : 0u)), dim3(64), 0, stream, c);
        ZK_LAUNCH(zkwitdev::k_wit_mul_affine, dim3(b64, zkwitdev::N_MULS * zkwitdev::MUL_SEGS), dim3(64), 0, stream, c);
        ZK_LAUNCH(zkwitdev::k_wit_mul_fill, dim3(b64, zkwitdev::N_MULS * zkwitdev::MUL_FILL_CHUNKS), dim3(64), 0, stream, c);
        ZK_LAUNCH(zkwitdev::k_wit_level2, dim3(b64, zkwitdev::L2_ROLES), dim3(64), 0, stream, c);
    }
    return witness_slot_end(R, np, slot, stream);
}
// waits for the witness kernels of `slot`; a malformed statement is reported with its absolute index
zk_status witness_gpu_finish(zk_r1cs* R, size_t np, int slot, size_t index_base) {
    HIP_TRY(hipEventSynchronize(R->work.wit_done[slot]));
    const uint32_t* bad = R->work.pin_bad[slot].as<uint32_t>();
    static const char* const points[5] = {"proof_generation_key", "enc_key_recipient", "enc_balance_left", "enc_balance_right", "g_epoch"};
    static const char* const scalars[3] = {"randomness", "alpha", "dec_key_sender"};
    for (size_t i = 0; i < np; i++) {
        if (!bad[i]) continue;
        const std::string who = "statement " + std::to_string(index_base + i) + ": ";
        // the order the host calculator checks them in (transfer_decode)
        for (int k = 0; k < 3; k++)
            if (bad[i] & (1u << (8 + k))) return fail(ZK_ERR_INVALID_ARGUMENT, who + scalars[k] + " is not a canonical Fs scalar");
        for (int k = 0; k < 5; k++)
            if (bad[i] & (2u << k)) return fail(ZK_ERR_INVALID_ARGUMENT, who + points[k] + " is not a Jubjub point");
        for (int k = 0; k < 5; k++)
            if (bad[i] & (1u << (zkwitdev::BAD_NOT_PRIME_ORDER + k)))
                return fail(ZK_ERR_INVALID_ARGUMENT, who + points[k] + " is not in the prime-order subgroup");
        return fail(ZK_ERR_INVALID_ARGUMENT, who + "malformed");
    }
    return ZK_OK;
}


// ---- the anonymous-transfer circuit (witness_anon_gpu.h): np statements -> R->work.z[slot], enqueued on `stream`.  The
// handle's witness buffers are shared with the transfer generator (a zk_r1cs holds ONE circuit).
zk_status witness_anon_gpu_enqueue(zk_r1cs* R, const zk_anonymous_statement* st, size_t np, int slot, hipStream_t stream) {
    using namespace zkwitdev;
    static_assert(sizeof(AStmt) == sizeof(zk_anonymous_statement), "statement layout");
    const SlotSizes S = {A_NV, sizeof(AStmt), AP_COUNT, A1_ROLES};
    ZK_TRY(witness_slot_stage(R, S, st, np, slot));
    // A member index out of range is reported by witness_anon_gpu_finish, in statement order with everything else the
    // kernels find - exactly where the host calculator reports it (statement_route.h anonymous_decode; ADVICE r4: refused
    // here, a bad index in chunk k + 1 was reported before chunk k had been proved).  The kernels see the index clamped.
    R->work.anon_index_bad[slot] = (size_t)-1;
    zk_anonymous_statement* ps = (zk_anonymous_statement*)R->work.pin_st[slot].p;
    for (size_t i = 0; i < np; i++)
        if (ps[i].s_index >= ZK_ANONYMOUS_SIZE || ps[i].t_index >= ZK_ANONYMOUS_SIZE) {
            if (R->work.anon_index_bad[slot] == (size_t)-1) R->work.anon_index_bad[slot] = i;
            ps[i].s_index = 0;
            ps[i].t_index = 1;
        }
    ACtx c;
    ZK_TRY(witness_slot_begin(R, S, np, slot, stream, 0xff, &c));   // A_BAD_NONE
    c.ast = R->work.wit_st[slot].as<AStmt>();
    const unsigned b64 = (unsigned)((np + 63) / 64);
    {
        ProfScope ps("witness_gpu", stream);
        ZK_LAUNCH(k_awit_decode, dim3((unsigned)((np * (2 + 4 * ANON) + 63) / 64)), dim3(64), 0, stream, c);
        ZK_LAUNCH(k_awit_level1, dim3(b64, A1_ROLES), dim3(64), 0, stream, c);
        ZK_LAUNCH(k_awit_mul_affine, dim3(b64, (ANON + 1) * MUL_SEGS), dim3(64), 0, stream, c, 0u);
        ZK_LAUNCH(k_awit_mul_fill, dim3(b64, (ANON + 1) * MUL_FILL_CHUNKS), dim3(64), 0, stream, c, 0u);
        ZK_LAUNCH(k_awit_level2, dim3(b64, A2_ROLES), dim3(64), 0, stream, c);
        ZK_LAUNCH(k_awit_level3, dim3(b64, 2), dim3(64), 0, stream, c);
        ZK_LAUNCH(k_awit_mul_affine, dim3(b64, MUL_SEGS), dim3(64), 0, stream, c, A_MUL_CRD_SK);
        ZK_LAUNCH(k_awit_mul_fill, dim3(b64, MUL_FILL_CHUNKS), dim3(64), 0, stream, c, A_MUL_CRD_SK);
        ZK_LAUNCH(k_awit_level4, dim3(b64), dim3(64), 0, stream, c);
    }
    return witness_slot_end(R, np, slot, stream);
}
// waits for the witness kernels of `slot`; a malformed statement is reported with its absolute index, in the words and the
// order of the host calculator (statement_route.h anonymous_decode)
zk_status witness_anon_gpu_finish(zk_r1cs* R, size_t np, int slot, size_t index_base) {
    using namespace zkwitdev;
    HIP_TRY(hipEventSynchronize(R->work.wit_done[slot]));
    const uint32_t* bad = R->work.pin_bad[slot].as<uint32_t>();
    static const char* const scalars[3] = {"randomness", "alpha", "dec_key"};
    static const char* const sets[4] = {"enc_keys", "left_ciphertexts", "enc_balances_left", "enc_balances_right"};
    for (size_t i = 0; i < np; i++) {
        // (the index check comes first inside a statement, as in anonymous_decode)
        if (i == R->work.anon_index_bad[slot])
            return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index_base + i) + ": member index out of range");
        const uint32_t code = bad[i];
        if (code == A_BAD_NONE) continue;
        const std::string who = "statement " + std::to_string(index_base + i) + ": ";
        if (code <= A_BAD_DEC_KEY) return fail(ZK_ERR_INVALID_ARGUMENT, who + scalars[code] + " is not a canonical Fs scalar");
        if (code == A_BAD_PGK) return fail(ZK_ERR_INVALID_ARGUMENT, who + "proof_generation_key is not a Jubjub point");
        if (code == A_BAD_GEPOCH) return fail(ZK_ERR_INVALID_ARGUMENT, who + "g_epoch is not a Jubjub point");
        const uint32_t k = (code - A_BAD_SET) / 4, set = (code - A_BAD_SET) % 4;
        return fail(ZK_ERR_INVALID_ARGUMENT, who + sets[set] + "[" + std::to_string(k) + "] is not a Jubjub point");
    }
    return ZK_OK;
}


// ---- ElGamal decryption (elgamal_dlog.h): the tables of a zk_elgamal_table and the search, on the library's stream
// xy[j] = j (2^shift G) for j < 2^count_log (k_dlog_multiples; its walk's Zs in a scratch released here)
static zk_status dlog_multiples(const zk_elgamal_table* T, uint32_t* xy, uint32_t count_log, uint32_t shift) {
    using namespace zkdlog;
    const uint32_t lanes_log = std::min(count_log, BUILD_LANES_LOG);
    DevBuf scratch;
    scratch.is_public = true;
    ZK_TRY(scratch.ensure((size_t)64 << count_log));
    {
        ProfScope ps("elgamal_table", g_stream);
        ZK_LAUNCH(k_dlog_multiples, dim3(((1u << lanes_log) + 63) / 64), dim3(64), 0, g_stream, xy, scratch.as<uint32_t>(),
                  T->consts.as<uint32_t>(), shift, lanes_log, 1u << (count_log - lanes_log));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
}
static zkdlog::Table dlog_table(const zk_elgamal_table* T) {
    zkdlog::Table t;
    t.xy = T->baby_xy.as<uint32_t>();
    t.slots = T->slots.as<unsigned long long>();
    t.slot_mask = (2u << T->baby_bits) - 1u;
    t.fp_mask = T->fp_bits >= 32 ? 0xffffffffu : (1u << T->fp_bits) - 1u;
    return t;
}
zk_status elgamal_table_build(zk_elgamal_table* T) {
    using namespace zkdlog;
    const uint32_t b = T->baby_bits;
    // G, 2 d and -M = -(2^b G), the layout of elgamal_dlog.h's consts
    const zkwit::JPoint g = zkwit::tables().win[0][1];
    zkwit::EPoint m = zkwit::to_ext(g);
    for (uint32_t k = 0; k < b; k++) m = zkwit::ext_add(m, m);
    zkwit::JPoint ma;
    zkwit::batch_to_affine(&m, &ma, 1);
    const zkhost::Fr c[5] = {g.x, g.y, zkwit::edwards_d().dbl(), zkhost::Fr::zero() - ma.x, ma.y};
    static_assert(sizeof(c) == C_WORDS * 4, "consts layout");
    ZK_TRY(T->consts.ensure(sizeof(c)));
    HIP_TRY(hipMemcpy(T->consts.p, c, sizeof(c), hipMemcpyHostToDevice));
    const size_t count = (size_t)1 << b;
    ZK_TRY(T->baby_xy.ensure(count * 64));
    ZK_TRY(T->slots.ensure(count * 16));   // 2^(b+1) slots of 8 bytes: half of them stay empty
    HIP_TRY(hipMemsetAsync(T->slots.p, 0, count * 16, g_stream));
    ZK_TRY(dlog_multiples(T, T->baby_xy.as<uint32_t>(), b, 0));
    {
        ProfScope ps("elgamal_table", g_stream);
        ZK_LAUNCH(k_dlog_insert, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, g_stream, dlog_table(T), (uint32_t)count);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
}
// the search over the nb points resident in T->v
static zk_status dlog_search_rows(zk_elgamal_table* T, size_t nb, uint64_t limit, uint64_t* x_out) {
    using namespace zkdlog;
    const uint32_t b = T->baby_bits, w = giant_stride_log(b);
    const uint64_t steps = (limit + (1ull << b) - 1) >> b;
    const uint32_t chunks = (uint32_t)((steps + (1ull << w) - 1) >> w);   // <= 2^16 (giant_stride_log)
    if (steps > 1 && chunks > T->giant_count) {   // the giant-step table: e 2^w M for e < the next power of two
        uint32_t log = 0;
        while ((1u << log) < chunks) log++;
        T->giant_count = 0;
        ZK_TRY(T->giant_xy.ensure((size_t)64 << log));
        ZK_TRY(dlog_multiples(T, T->giant_xy.as<uint32_t>(), log, b + w));
        T->giant_count = 1u << log;
    }
    ZK_TRY(T->res.ensure(nb * 8));
    Search s;
    s.tab = dlog_table(T);
    s.v = T->v.as<uint32_t>();
    s.giant = T->giant_xy.as<uint32_t>();
    s.consts = T->consts.as<uint32_t>();
    s.scratch = nullptr;
    s.res = T->res.as<unsigned long long>();
    s.limit = limit;
    s.steps = steps;
    s.n = (uint32_t)nb;
    s.baby_bits = b;
    s.w_log = w;
    s.chunks = chunks;
    s.lanes = 0;
    HIP_TRY(hipMemsetAsync(T->res.p, 0xff, nb * 8, g_stream));   // NOT_FOUND
    size_t scratch_used = 0;
    {
        ProfScope ps("elgamal_dlog", g_stream);
        if (steps == 1) {   // limit <= 2^b: the table holds the whole range
            ZK_LAUNCH(k_dlog_probe, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, g_stream, s);
        } else {
            const uint64_t items = (uint64_t)nb * chunks;
            s.lanes = (uint32_t)std::min<uint64_t>((items + 63) / 64 * 64, SEARCH_LANES);
            scratch_used = (size_t)s.lanes * SEARCH_BATCH * 4 * 32;
            ZK_TRY(T->scratch.ensure(scratch_used));
            s.scratch = T->scratch.as<uint32_t>();
            ZK_LAUNCH(k_dlog_search, dim3(s.lanes / 64), dim3(64), 0, g_stream, s);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x_out, T->res.p, nb * 8, hipMemcpyDeviceToHost, g_stream));
    // the key-derived points do not stay on the device between calls
    HIP_TRY(hipMemsetAsync(T->v.p, 0, nb * 64, g_stream));
    if (scratch_used) HIP_TRY(hipMemsetAsync(T->scratch.p, 0, scratch_used, g_stream));
    HIP_TRY(hipMemsetAsync(T->res.p, 0, nb * 8, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
}
zk_status elgamal_dlog_search_resident(zk_elgamal_table* T, size_t nb, uint64_t limit, uint64_t* x_out) {
    static_assert(sizeof(zkhost::Fr) == 32 && sizeof(unsigned long long) == sizeof(uint64_t), "layouts");
    const zk_status rc = dlog_search_rows(T, nb, limit, x_out);
    if (rc != ZK_OK) {   // (a failure before the wipes above: the points are in T->v already)
        (void)hipMemsetAsync(T->v.p, 0, nb * 64, g_stream);
        (void)hipStreamSynchronize(g_stream);
    }
    return rc;
}
zk_status elgamal_dlog_search(zk_elgamal_table* T, size_t n, const zkhost::Fr* v, uint64_t limit, uint64_t* x_out) {
    for (size_t first = 0; first < n; first += ELGAMAL_SEARCH_BLOCK) {
        const size_t nb = std::min(ELGAMAL_SEARCH_BLOCK, n - first);
        ZK_TRY(T->v.ensure(nb * 64));
        HIP_TRY(hipMemcpyAsync(T->v.p, v + first * 2, nb * 64, hipMemcpyHostToDevice, g_stream));
        ZK_TRY(elgamal_dlog_search_resident(T, nb, limit, x_out + first));
    }
    return ZK_OK;
}
