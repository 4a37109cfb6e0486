// libzkamd, the statement route: what lies between a batch of statements of a built-in circuit (the confidential transfer, the
// anonymous transfer) and prove_from_z, written once for both - the host witness calculators behind the C ABI, one description
// per circuit, the checks of a (key, circuit) pair, the chunk loop over either witness engine, the read-back of the witness
// kernels' vectors and the natively emitted constraint systems.  Part of zkamd.cpp's translation unit (included by it alone,
// behind prove_from_z and prove_batch_witness).
#pragma once
#include "prover_binding.h"
#include "pipeline_lanes.h"   // (SlotThread: the helper thread of the host engine)

// ------------------------------------------------------------------------------------------
// the witness calculators of the two circuits (transfer_witness.h) behind the C ABI
// ------------------------------------------------------------------------------------------
namespace {

zk_status decode_fs(const uint8_t* b, uint64_t (&v)[4], size_t index, const char* what) {
    static const uint64_t FS[4] = ZK_JUBJUB_FS_MODULUS_64;
    load_scalar_le(b, v);
    for (int i = 3; i >= 0; i--) {
        if (v[i] < FS[i]) return ZK_OK;
        if (v[i] > FS[i]) break;
    }
    return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index) + ": " + what + " is not a canonical Fs scalar");
}
zk_status decode_jubjub(const uint8_t* b, zkwit::JPoint* p, size_t index, const std::string& what) {
    if (!zkwit::decode_point(b, p))
        return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index) + ": " + what + " is not a Jubjub point");
    return ZK_OK;
}

zk_status transfer_decode(const zk_transfer_statement& in, size_t index, zkwit::Statement* out) {
    out->amount = in.amount;
    out->remaining_balance = in.remaining_balance;
    out->fee = in.fee;
    ZK_TRY(decode_fs(in.randomness, out->randomness, index, "randomness"));
    ZK_TRY(decode_fs(in.alpha, out->alpha, index, "alpha"));
    ZK_TRY(decode_fs(in.dec_key_sender, out->dec_key, index, "dec_key_sender"));
    ZK_TRY(decode_jubjub(in.proof_generation_key, &out->pgk, index, "proof_generation_key"));
    ZK_TRY(decode_jubjub(in.enc_key_recipient, &out->enc_key_recipient, index, "enc_key_recipient"));
    ZK_TRY(decode_jubjub(in.enc_balance_left, &out->enc_balance_left, index, "enc_balance_left"));
    ZK_TRY(decode_jubjub(in.enc_balance_right, &out->enc_balance_right, index, "enc_balance_right"));
    ZK_TRY(decode_jubjub(in.g_epoch, &out->g_epoch, index, "g_epoch"));
    return ZK_OK;
}

zk_status anonymous_decode(const zk_anonymous_statement& in, size_t index, zkwit::AnonStatement* out) {
    if (in.s_index >= ZK_ANONYMOUS_SIZE || in.t_index >= ZK_ANONYMOUS_SIZE)
        return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index) + ": member index out of range");
    out->amount = in.amount;
    out->remaining_balance = in.remaining_balance;
    out->s_index = in.s_index;
    out->t_index = in.t_index;
    ZK_TRY(decode_fs(in.randomness, out->randomness, index, "randomness"));
    ZK_TRY(decode_fs(in.alpha, out->alpha, index, "alpha"));
    ZK_TRY(decode_fs(in.dec_key, out->dec_key, index, "dec_key"));
    ZK_TRY(decode_jubjub(in.proof_generation_key, &out->pgk, index, "proof_generation_key"));
    ZK_TRY(decode_jubjub(in.g_epoch, &out->g_epoch, index, "g_epoch"));
    for (size_t k = 0; k < ZK_ANONYMOUS_SIZE; k++) {
        const std::string m = "[" + std::to_string(k) + "]";
        ZK_TRY(decode_jubjub(in.enc_keys[k], &out->enc_keys[k], index, "enc_keys" + m));
        ZK_TRY(decode_jubjub(in.left_ciphertexts[k], &out->left_ciphertexts[k], index, "left_ciphertexts" + m));
        ZK_TRY(decode_jubjub(in.enc_balances_left[k], &out->balance_left[k], index, "enc_balances_left" + m));
        ZK_TRY(decode_jubjub(in.enc_balances_right[k], &out->balance_right[k], index, "enc_balances_right" + m));
    }
    return ZK_OK;
}

// n statements -> n variable assignments on the host cores.  decode(i, &statement) / synth(statement, wit).
template <class Stmt, class Decode, class Synth>
zk_status witness_batch(size_t n, size_t n_inputs, size_t n_aux, uint32_t flags, uint8_t* out, Decode&& decode, Synth&& synth) {
    // decode(i, ...) reports the ABSOLUTE statement index (the callers add their batch offset); threads own
    // increasing index ranges and stop at their first failure, so the first failing thread holds the
    // lowest failing statement
    if (n == 0) return ZK_OK;
    (void)zkwit::tables();   // build the window tables before the threads start
    const size_t nv = n_inputs + n_aux;
    const unsigned nthreads = host_threads(n, 64);
    std::vector<zk_status> sts(nthreads, ZK_OK);
    std::vector<std::string> msgs(nthreads);
    const bool mont = (flags & ZK_FR_MONTGOMERY) != 0;
    auto work = [&](unsigned t) {
        for (size_t i = n * t / nthreads; i < n * (t + 1) / nthreads; i++) {
            Stmt s;
            zk_status rc = decode(i, &s);
            if (rc != ZK_OK) {
                sts[t] = rc;
                msgs[t] = g_err;
                return;
            }
            zkwit::Wit w;
            synth(s, w);
            if (w.inputs.size() != n_inputs || w.aux.size() != n_aux) {
                sts[t] = ZK_ERR_INVALID_ARGUMENT;
                msgs[t] = "internal: witness size mismatch";
                return;
            }
            uint64_t* dst = reinterpret_cast<uint64_t*>(out + i * nv * 32);
            size_t k = 0;
            for (const auto* vec : {&w.inputs, &w.aux})
                for (const zkhost::Fr& v : *vec) {
                    zkhost::Fr x = mont ? v : v.from_mont();
                    memcpy(dst + 4 * k, x.l, 32);
                    k++;
                }
        }
    };
    run_threads(nthreads, work);
    for (unsigned t = 0; t < nthreads; t++)
        if (sts[t] != ZK_OK) return fail(sts[t], msgs[t]);
    return ZK_OK;
}

// index_base: the place of st[0] in the caller's batch (a malformed statement is reported with its absolute index)
zk_status transfer_witness(const zk_transfer_statement* st, size_t n, uint32_t flags, uint8_t* out, size_t index_base = 0) {
    if ((!st || !out) && n) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return witness_batch<zkwit::Statement>(
        n, ZK_TRANSFER_N_INPUTS, ZK_TRANSFER_N_AUX, flags, out,
        [&](size_t i, zkwit::Statement* s) { return transfer_decode(st[i], index_base + i, s); },
        [n](const zkwit::Statement& s, zkwit::Wit& w) {
            // fewer statements than a fifth of the host threads: each statement's five 252-bit multiplications side by side
            // (transfer_witness.h synthesize_parallel) - one transaction 1.2 -> 0.35 ms; a batch keeps one thread per statement
            if (n * 5 <= (size_t)host_threads(64, 64)) zkwit::synthesize_parallel(s, w);
            else zkwit::synthesize(s, w);
        });
}
zk_status anonymous_witness(const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* out, size_t index_base = 0) {
    if ((!st || !out) && n) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    static_assert(zkwit::ANON_SIZE == ZK_ANONYMOUS_SIZE, "anonymity set size");
    return witness_batch<zkwit::AnonStatement>(
        n, ZK_ANONYMOUS_N_INPUTS, ZK_ANONYMOUS_N_AUX, flags, out,
        [&](size_t i, zkwit::AnonStatement* s) { return anonymous_decode(st[i], index_base + i, s); },
        [](const zkwit::AnonStatement& s, zkwit::Wit& w) { zkwit::synthesize_anonymous(s, w); });
}

// Which engine computes the variable assignment of n statements.  ZKAMD_WITNESS = host | gpu forces one.  Default: the GPU
// generator (witness_gpu.h) - except for a handful of statements: its kernels are serial chains (point decompression 2.0 ms,
// the 252-bit in-circuit multiplications 5.1 + 0.7 ms, the rest 0.7) that take 8.4 ms whatever the batch holds, while the
// native host calculator (transfer_witness.h) needs 1.4 ms per statement and host thread.  A transaction proved ALONE - the
// reference's call pattern, one gen_proof per transfer - is 11.5 ms through the kernels and 4.6 ms with its assignment
// computed on a host core, as the reference's own synthesize is (profiles/r05_experiments.txt r05k / r05l).  The proof itself
// (create_proof) is on the GPU either way.  n = SIZE_MAX: a stream of batches (zk_pipeline) - the GPU generator.
bool witness_on_host(size_t n = (size_t)-1) {
    if (const char* env = getenv("ZKAMD_WITNESS")) {
        if (!strcmp(env, "host")) return true;
        if (!strcmp(env, "gpu")) return false;
    }
    // (the crossover, measured with 16 host threads: 64 statements 34.0 against 39.3 ms per call, 128: 51.9 / 53.9, 192: 68.2 / 69.3,
    //  256: 87.6 / 85.3 - tools/witness_engine_probe.py, profiles/r05end_witness_engine_probe.txt)
    return n != (size_t)-1 && n <= 8 * (size_t)host_threads(n, 64);
}

// ------------------------------------------------------------------------------------------
// one description per built-in circuit, indexed by zkpairs::Circuit
// ------------------------------------------------------------------------------------------
struct StatementRoute {
    uint32_t n_in, n_aux;
    size_t st_size;      // sizeof the statement of the C ABI
    const char* name;    // as the refusal of other matrices names the circuit
    size_t chunk_cap;    // proofs per launch set at the most (0: ProveTunables' alone)
    // the witness kernels of np statements into R->work.z[slot], enqueued on `stream` / awaited (witness.cpp).  typed_inputs: a
    // wallet-level request's points are tested for prime order too (the anonymous entry checks them on the host: ignored)
    zk_status (*gpu_enqueue)(zk_r1cs* R, const void* st, size_t np, int slot, hipStream_t stream, bool typed_inputs);
    zk_status (*gpu_finish)(zk_r1cs* R, size_t np, int slot, size_t index_base);
    // the host calculator above
    zk_status (*host_witness)(const void* st, size_t n, uint32_t flags, uint8_t* out, size_t index_base);

    size_t nv() const { return (size_t)n_in + n_aux; }
    size_t chunk() const {
        const size_t c = ProveTunables::read().batch_chunk;
        return chunk_cap && c > chunk_cap ? chunk_cap : c;
    }
};
static_assert(zkpairs::TRANSFER == 0 && zkpairs::ANONYMOUS == 1, "the order of the descriptions");
const StatementRoute STATEMENT_ROUTES[2] = {
    {ZK_TRANSFER_N_INPUTS, ZK_TRANSFER_N_AUX, sizeof(zk_transfer_statement), "transfer", 0,
     [](zk_r1cs* R, const void* st, size_t np, int slot, hipStream_t s, bool typed) { return witness_gpu_enqueue(R, (const zk_transfer_statement*)st, np, slot, s, typed); },
     witness_gpu_finish,
     [](const void* st, size_t n, uint32_t f, uint8_t* out, size_t base) { return transfer_witness((const zk_transfer_statement*)st, n, f, out, base); }},
    // (domain 2^16: half the proofs of a transfer chunk fill the same workspaces)
    {ZK_ANONYMOUS_N_INPUTS, ZK_ANONYMOUS_N_AUX, sizeof(zk_anonymous_statement), "anonymous-transfer", 512,
     [](zk_r1cs* R, const void* st, size_t np, int slot, hipStream_t s, bool) { return witness_anon_gpu_enqueue(R, (const zk_anonymous_statement*)st, np, slot, s); },
     witness_anon_gpu_finish,
     [](const void* st, size_t n, uint32_t f, uint8_t* out, size_t base) { return anonymous_witness((const zk_anonymous_statement*)st, n, f, out, base); }},
};

}  // namespace

// What every entry of the route refuses of a (key, circuit) pair, in this order: matrices of another shape than the circuit's;
// handles on different devices; nothing more of an empty batch (n = 0: the caller returns ZK_OK); then, on the pair's device
// (made current here), more rows than the key's evaluation domain.  P = null: the circuit alone (the read-back entries).
zk_status zkrt::route_check(zk_params* P, zk_r1cs* R, int circuit, size_t n) {
    const StatementRoute& T = STATEMENT_ROUTES[circuit];
    if (R->sys.n_in != T.n_in || R->sys.n_aux != T.n_aux)
        return fail(ZK_ERR_INVALID_ARGUMENT, std::string("the loaded constraint matrices are not the ") + T.name + " circuit's");
    if (P && R->sys.device != P->key.device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(P ? P->key.device : R->sys.device));
    if (P && (size_t)R->sys.n_con + R->sys.n_in > P->key.m)
        return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    return ZK_OK;
}

namespace {

// The witnesses of a run of chunks over two slots, by either engine, so that chunk k + 1 is made while the GPU works on chunk k:
//   the witness kernels (witness_gpu.h / witness_anon_gpu.h), on the side stream of the copy engine: latency-bound chains for a
//     few hundred waves beside the multiexps; a slot is R->work.z[slot];
//   a handful of statements, or ZKAMD_WITNESS=host (witness_on_host): the host calculator on the host cores, in a thread beside
//     the caller; a slot is one half (chunk_capacity assignments) of the pinned R->work.host_z.
// start() may come before ready() of the chunk before it (zk_pipeline) or after it (statement_chunks): start() waits for the one
// helper thread, whose result is kept per slot, and ready() waits only while the thread is still on the slot asked for - so the
// next chunk's witnesses are made beside the current chunk's proving in either order.
struct ChunkWitness {
    zk_r1cs* const R;
    const StatementRoute& T;
    const bool host, typed_inputs;
    const size_t half;
    zk_status side_rc[2] = {ZK_OK, ZK_OK};   // what the helper thread made of a slot, with its message (g_err is thread-local)
    std::string side_err[2];
    zkpipe::SlotThread side;   // (behind what it writes: joined first as this goes)
    ChunkWitness(zk_r1cs* R, const StatementRoute& T, bool host, size_t chunk_capacity, bool typed_inputs)
        : R(R), T(T), host(host), typed_inputs(typed_inputs), half(chunk_capacity * T.nv() * 32) {}
    // index_base: the place of st[0] in the caller's batch (a malformed statement is reported with its absolute index)
    zk_status start(const void* st, size_t np, int slot, size_t index_base) {
        if (!host) return T.gpu_enqueue(R, st, np, slot, g_copy_stream, typed_inputs);
        side.join();   // (before the buffer may move)
        // (never cached: another entry on this handle may have regrown the buffer since; it only grows, so not under a half in use)
        ZK_TRY(R->work.host_ensure(2 * half));
        uint8_t* const out = (uint8_t*)R->work.host_z + slot * half;
        side.start(slot, [this, st, np, slot, index_base, out] {
            side_rc[slot] = guarded([&] { return T.host_witness(st, np, ZK_FR_MONTGOMERY, out, index_base); });
            if (side_rc[slot] != ZK_OK) side_err[slot] = g_err;
        });
        return ZK_OK;
    }
    zk_status ready(size_t np, int slot, size_t index_base) {
        if (!host) return T.gpu_finish(R, np, slot, index_base);
        side.join_slot(slot);
        return side_rc[slot] == ZK_OK ? ZK_OK : fail(side_rc[slot], side_err[slot]);
    }
    // the slot's assignments where the host engine made them (Montgomery form), null where the kernels left them in R->work.z[slot]
    const uint8_t* host_z(int slot) const { return host ? (const uint8_t*)R->work.host_z + slot * half : nullptr; }
    // behind an error: no witness kernel of a later chunk stays in flight, nor its thread
    void drain() {
        side.join();
        const std::string why = g_err;
        (void)hipStreamSynchronize(g_copy_stream);
        g_err = why;
    }
};

// The chunk loop of the statement entries, n > 0 statements behind route_check, in chunks of the circuit's launch set: the
// witnesses of chunk k + 1 are made while step(first, np, slot, host_z) works on chunk k, and a malformed statement among them
// is reported once chunk k is done.  host_z: ChunkWitness::host_z of the slot.
template <class Step>
zk_status statement_chunks(zk_r1cs* R, zkpairs::Circuit circuit, const void* st, size_t n, Step&& step, bool typed_inputs = false) {
    const StatementRoute& T = STATEMENT_ROUTES[circuit];
    const size_t chunk = T.chunk();
    ChunkWitness W(R, T, witness_on_host(n), std::min(chunk, n), typed_inputs);
    auto at = [&](size_t first) { return (const uint8_t*)st + first * T.st_size; };
    zk_status rc = W.start(at(0), std::min(chunk, n), 0, 0);
    int slot = 0;
    for (size_t first = 0; first < n && rc == ZK_OK; first += chunk, slot ^= 1) {
        const size_t np = std::min(chunk, n - first), next = first + chunk;
        rc = W.ready(np, slot, first);
        if (rc == ZK_OK && next < n) rc = W.start(at(next), std::min(chunk, n - next), slot ^ 1, next);
        if (rc == ZK_OK) rc = step(first, np, slot, W.host_z(slot));
    }
    if (rc != ZK_OK) W.drain();
    return rc;
}

// Statements -> proofs: a chunk's step is row evaluations + create_proof over the derived bases of the pair
zk_status prove_statements(zk_params* P, zk_r1cs* R, zkpairs::Circuit circuit, const void* st, size_t n, const uint8_t* rs, uint8_t* out) {
    return statement_chunks(R, circuit, st, n, [&](size_t first, size_t np, int slot, const uint8_t* host_z) {
        return host_z ? prove_batch_witness(P, R, np, host_z, ZK_FR_MONTGOMERY, rs + first * 64, out + first * 192, true)
                      : prove_from_z(P, R, np, slot, rs + first * 64, out + first * 192, true);
    });
}

// Statements -> verdicts: a chunk's step is the constraint check (r1cs_check.h) of its assignments - the host engine's uploaded
// into R->work.z[0] first, the same kernel over either
zk_status check_statements(zk_r1cs* R, zkpairs::Circuit circuit, const void* st, size_t n, zk_r1cs_verdict* out) {
    return statement_chunks(R, circuit, st, n, [&](size_t first, size_t np, int slot, const uint8_t* host_z) {
        return host_z ? check_batch_witness(R, np, host_z, ZK_FR_MONTGOMERY, out + first, true) : check_from_z(R, np, slot, out + first);
    });
}

// The witness vectors the GPU generator of a circuit produces, copied back to the host: lets the tests compare it with the
// host calculator element by element.  out: n x (n_in + n_aux) x 32 bytes.
zk_status witness_readback(zk_r1cs* R, zkpairs::Circuit circuit, const void* st, size_t n, uint32_t flags, uint8_t* out) {
    if (!R || (n && (!st || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(nullptr, R, circuit));
    const StatementRoute& T = STATEMENT_ROUTES[circuit];
    const size_t nv = T.nv(), chunk = std::min(T.chunk(), (size_t)256);
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        ZK_TRY(T.gpu_enqueue(R, (const uint8_t*)st + first * T.st_size, np, 0, g_stream, false));
        ZK_TRY(T.gpu_finish(R, np, 0, first));
        if (!(flags & ZK_FR_MONTGOMERY)) {
            const size_t cnt = np * nv;
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, R->work.z[0].as<uint32_t>(),
                      (const uint32_t*)R->work.z[0].as<uint32_t>(), 1u, cnt, (uint32_t*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipMemcpy(out + first * nv * 32, R->work.z[0].p, np * nv * 32, hipMemcpyDeviceToHost));
    }
    return ZK_OK;
}

// the natively emitted constraint system of a circuit (transfer_r1cs.h; prover_binding.h builtin_system: built once per process)
zk_status system_fingerprint(zkpairs::Circuit circuit, uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints) {
    const zkr1cs::System& sys = builtin_system(circuit);
    if (hash_out) sys.fingerprint(hash_out);
    if (n_inputs) *n_inputs = sys.n_inputs;
    if (n_aux) *n_aux = sys.n_aux;
    if (n_constraints) *n_constraints = sys.n_constraints;
    return ZK_OK;
}
zk_status system_load(zkpairs::Circuit circuit, int device, zk_r1cs** out) {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const zkr1cs::System& sys = builtin_system(circuit);
    if (sys.n_inputs != STATEMENT_ROUTES[circuit].n_in || sys.n_aux != STATEMENT_ROUTES[circuit].n_aux)
        return fail(ZK_ERR_INVALID_ARGUMENT, "internal: emitted system has the wrong shape");
    std::vector<uint8_t> coeff[3];
    zk_csr mats[3];
    for (int m = 0; m < 3; m++) {
        const zkr1cs::Csr& M = sys.m[m];
        coeff[m].resize(M.coeff.size() * 32 + 32);
        for (size_t k = 0; k < M.coeff.size(); k++) {
            const zkhost::Fr p = M.coeff[k].from_mont();
            memcpy(&coeff[m][k * 32], p.l, 32);
        }
        mats[m].row_ptr = M.row_ptr.data();
        mats[m].col = M.col.data();
        mats[m].coeff = coeff[m].data();
    }
    const zk_csr* ptrs[3] = {&mats[0], &mats[1], &mats[2]};
    std::vector<uint32_t> stage_first;   // the parts of the circuit, for zk_r1cs_stage
    std::vector<std::string> stage_name;
    for (const auto& mk : sys.marks) {
        stage_first.push_back(mk.first);
        stage_name.push_back(mk.second);
    }
    ZK_TRY(r1cs_load(sys.n_inputs, sys.n_aux, sys.n_constraints, ptrs, device, out));
    (*out)->sys.stage_first.swap(stage_first);
    (*out)->sys.stage_name.swap(stage_name);
    return ZK_OK;
}

}  // namespace
