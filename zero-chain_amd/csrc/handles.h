// Handle types shared by the translation units of libzkamd.
#pragma once
#include <chrono>
#include <functional>
#include <vector>
#include "host_common.h"
#include "host_math.h"

// ------------------------------------------------------------------------------------------
// zk_r1cs: the fixed constraint matrices of a circuit, resident on the GPU
// ------------------------------------------------------------------------------------------
struct zk_r1cs {
    // What r1cs_load made of the caller's matrices.  Another lane of a pipeline shares it (share below).
    struct System {
        int device = 0;
        uint32_t n_in = 0, n_aux = 0, n_con = 0;
        uint64_t id = 0;   // one per loaded system (a lane's clone keeps it): what a key's derived bases are bound to
        zkrt::DevBuf row_ptr[3], col[3], coeff[3];
        std::vector<uint8_t> a_aux_density, b_input_density, b_aux_density;
        // host copy of the matrices (the parameter generator transposes them): CSR, Montgomery coefficients
        std::vector<uint32_t> h_row_ptr[3], h_col[3];
        std::vector<zkhost::Fr> h_coeff[3];
        // the parts of a built-in circuit (transfer_r1cs.h System::mark), ascending: stage k is the constraints
        // [stage_first[k], stage_first[k + 1]) - the last one ends at n_con.  Empty for matrices a caller loaded.
        std::vector<uint32_t> stage_first;
        std::vector<std::string> stage_name;
        // The matrices on the GPU borrowed, the shape and the densities copied; o must outlive this one.  The host copy stays
        // with o alone: a key is bound to the circuit through the handle that loaded it (ensure_derived does nothing without).
        void share(const System& o) {
            device = o.device;
            n_in = o.n_in; n_aux = o.n_aux; n_con = o.n_con;
            id = o.id;
            for (int m = 0; m < 3; m++) {
                row_ptr[m].borrow(o.row_ptr[m]);
                col[m].borrow(o.col[m]);
                coeff[m].borrow(o.coeff[m]);
            }
            a_aux_density = o.a_aux_density;
            b_input_density = o.b_input_density;
            b_aux_density = o.b_aux_density;
            stage_first = o.stage_first;
            stage_name = o.stage_name;
        }
    } sys;
    // What the proving calls on this handle fill.  Every handle has its own: a lane's clone starts with none.
    struct Work {
        // per-chunk workspaces: Montgomery assignment (two: the witness kernels fill one while the prover reads the
        // other), row evaluations
        zkrt::DevBuf z[2], abc;
        // the constraint check (r1cs_check.h): 16 bytes of flags over the caller's scalars | one verdict per assignment
        zkrt::DevBuf verdict;
        // GPU witness generator of the transfer circuit (witness_gpu.h)
        zkrt::DevBuf wit_st[2], wit_bad[2], wit_pts, wit_table, wit_consts, wit_scratch;
        zkrt::PinBuf pin_st[2], pin_bad[2];
        hipEvent_t wit_done[2] = {nullptr, nullptr};
        size_t anon_index_bad[2] = {(size_t)-1, (size_t)-1};   // first statement of the slot whose member indices are out of range
        bool wit_ready = false;
        // pinned host buffer of zk_transfer_prove_batch in host-witness mode (witness vectors of one chunk)
        void* host_z = nullptr;
        size_t host_z_cap = 0;
        Work() { verdict.is_public = true; }
        Work(const Work&) = delete;
        Work& operator=(const Work&) = delete;
        ~Work() {
            if (host_z) {
                explicit_bzero(host_z, host_z_cap);   // witness vectors: the bits of the keys
                (void)hipHostFree(host_z);
            }
            for (int k = 0; k < 2; k++)
                if (wit_done[k]) (void)hipEventDestroy(wit_done[k]);
        }
        zk_status host_ensure(size_t bytes) {
            if (bytes <= host_z_cap) return ZK_OK;
            if (host_z) {
                explicit_bzero(host_z, host_z_cap);
                (void)hipHostFree(host_z);
            }
            host_z = nullptr;
            host_z_cap = 0;
            if (hipHostMalloc(&host_z, bytes) != hipSuccess) {
                host_z = nullptr;
                return zkrt::fail(ZK_ERR_OUT_OF_MEMORY, "hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
            }
            host_z_cap = bytes;
            return ZK_OK;
        }
    } work;
};


// GPU witness generator of the transfer circuit (witness.cpp): np statements -> R->work.z[slot], enqueued on `stream`;
// finish() waits for it and reports a malformed statement with its absolute index
// typed_inputs: also run the reference's as_prime_order on the four points a wallet-level request brings in
zk_status witness_gpu_enqueue(zk_r1cs* R, const zk_transfer_statement* st, size_t np, int slot, hipStream_t stream,
                              bool typed_inputs = false);
zk_status witness_gpu_finish(zk_r1cs* R, size_t np, int slot, size_t index_base);
// ... and of the anonymous-transfer circuit (witness_anon_gpu.h)
zk_status witness_anon_gpu_enqueue(zk_r1cs* R, const zk_anonymous_statement* st, size_t np, int slot, hipStream_t stream);
zk_status witness_anon_gpu_finish(zk_r1cs* R, size_t np, int slot, size_t index_base);

// ------------------------------------------------------------------------------------------
// zk_elgamal_table: the baby steps of the discrete-log search behind zk_elgamal_decrypt (elgamal_dlog.h), resident on the GPU
// ------------------------------------------------------------------------------------------
constexpr uint32_t ELGAMAL_BABY_BITS_DEFAULT = 20, ELGAMAL_BABY_BITS_MIN = 8, ELGAMAL_BABY_BITS_MAX = 24;
struct zk_elgamal_table {
    int device = 0;
    uint32_t baby_bits = ELGAMAL_BABY_BITS_DEFAULT;
    uint32_t fp_bits = 32;       // fingerprint width of a hash slot (the test hooks shrink it to force false hits)
    uint32_t giant_count = 0;    // entries of the giant-step table built so far
    // public (multiples of the generator): G, 2 d, -2^b G | j G, j < 2^b | the hash | e 2^(b+w) G, e < giant_count
    zkrt::DevBuf consts, baby_xy, slots, giant_xy;
    // key-derived (left - dk right, the search's points, the logarithms): zeroed before release
    zkrt::DevBuf v, scratch, res;
    // the point stage of the scans and the balance query (wallet_stage.h device_stage, which alone lays them out).  Public chain
    // data: the encodings and the rows that pair them | their coordinates, statuses and what the combine leaves per row.
    // Key-derived: the digits of dk (a key set: the scalar of every hit) and dk * right
    zkrt::DevBuf scan_in, scan_out, scan_key;
    zk_elgamal_table() {
        consts.is_public = baby_xy.is_public = slots.is_public = giant_xy.is_public = scan_in.is_public = scan_out.is_public = true;
    }
};
// witness.cpp: build the baby-step table of T (baby_bits, fp_bits and device set); the search for n points v (affine,
// Montgomery x | y) over [0, limit): x_out[i] = the logarithm, or ~0 when there is none below the limit
zk_status elgamal_table_build(zk_elgamal_table* T);
zk_status elgamal_dlog_search(zk_elgamal_table* T, size_t n, const zkhost::Fr* v, uint64_t limit, uint64_t* x_out);
// ... and its second half alone: the nb <= ELGAMAL_SEARCH_BLOCK points are already in T->v, written on the library stream (by
// the copy of elgamal_dlog_search, or by k_scan_combine).  T->v is zeroed again on every way out.
constexpr size_t ELGAMAL_SEARCH_BLOCK = (size_t)1 << 20;   // points per launch
zk_status elgamal_dlog_search_resident(zk_elgamal_table* T, size_t nb, uint64_t limit, uint64_t* x_out);

// Groth16 verification of a batch (verify.cpp; zk_verify_batch is this with own_proofs = false).  own_proofs: the
// proofs are this library's own fresh results (gen_proof's self-check) - decoded without the r-torsion test.
namespace zkrt {
// what wallet.cpp (gen_proof, the Jubjub host side) needs of zkamd.cpp: the proofs of n > 0 transfer statements behind route_check,
// chunk by chunk (statement_route.h statement_chunks); packed(first, np, heads, head_stride) after each chunk is proved: the 23
// public inputs of its statement i at heads + i * head_stride, Montgomery form.  since: the ZKAMD_DEBUG_TIMING prints' zero, or null
using TransferChunkPacked = std::function<zk_status(size_t first, size_t np, const uint8_t* heads, size_t head_stride)>;
zk_status lib_transfer_chunks(zk_params* P, zk_r1cs* R, size_t n, const zk_transfer_statement* st, const uint8_t* rs, uint8_t* proofs_out,
                              const TransferChunkPacked& packed, const std::chrono::steady_clock::time_point* since);
bool lib_witness_on_host(size_t n);   // a handful of statements: the assignment on the host cores (statement_route.h witness_on_host)
// what every statement entry refuses of a (key, circuit) pair (statement_route.h): circuit = 0 the transfer circuit, 1 the
// anonymous one (zkpairs::Circuit); P = null: the circuit alone; n = 0: the checks of an empty batch, which come before the
// device is made current and the key's evaluation domain is compared
zk_status route_check(zk_params* P, zk_r1cs* R, int circuit, size_t n = 1);
zk_status verify_batch(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs, uint8_t* ok_out,
                       bool own_proofs, int form = VERIFY_AUTO, const uint8_t* own_affine = nullptr);
}
