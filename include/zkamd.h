/* zkamd.h - C ABI of the MI355X-native Groth16 prover hot path (libzkamd.so).
 *
 * Drop-in boundary for the ONE call LayerXcom/zero-chain makes into bellman on the proving
 * path:   create_random_proof(instance, &self.proving_key, rng)
 *           /root/reference/core/proofs/src/confidential.rs:149  (and anonymous.rs:165)
 * plus the Parameters load next to it (confidential.rs:95-103, Parameters::read(.., true)).
 *
 * The reference has no FFI today (the seam is a Rust generic call into the un-vendored bellman
 * 0.1.0 crate).  The entry points below are what a Rust `core/proofs` would bind with
 * `extern "C"` (see INTEGRATION.md for the stub): the Rust side keeps Circuit::synthesize and
 * its ProvingAssignment (host, witness generation) and hands the assignment to zk_prove*, which
 * replaces bellman's EvaluationDomain pipeline, its eight multiexp calls and the final fold.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every byte buffer; the library owns device
 *     memory behind the opaque handles; no exceptions or panics cross the ABI.
 *   - scalars (Fr) are 32 bytes little-endian.  By default they are PLAIN integers < r
 *     (FrRepr::write_le order, core/pairing/src/bls12_381/fr.rs:57-58); with ZK_FR_MONTGOMERY they
 *     are the raw in-memory Montgomery limbs of `Fr` (fr.rs:246-247), i.e. a Rust Vec<Fr> can be
 *     passed without conversion.
 *   - points use the reference's encodings: uncompressed G1 96 B / G2 192 B big-endian
 *     (core/pairing/src/bls12_381/ec.rs:666-753, :1303-1427) in Parameters, and a Proof is the
 *     192 bytes of Proof::write (core/bellman-verifier/src/lib.rs:55-65): A (G1 compressed 48 B)
 *     || B (G2 compressed 96 B) || C (G1 compressed 48 B).
 *   - status codes 1..8 map 1:1 onto bellman's SynthesisError variants
 *     (mirrored in-tree at core/bellman-verifier/src/lib.rs:359-383).
 *   - one handle may be used from one host thread at a time (the reference caller is
 *     single-threaded); different handles - on the same or on different GPUs - may be used from
 *     different threads: streams live in a per-device context, the current device is selected on
 *     every entry.
 *   - no C++ exception leaves the library: every entry that returns a zk_status is an exception barrier
 *     (a failed host allocation is ZK_ERR_OUT_OF_MEMORY, anything else ZK_ERR_DEVICE with the text in
 *     zk_last_error()), also for work the library does on its own threads.
 *
 * Index: entry point -> the reference interface it replaces (paths under /root/reference; "bellman" = the un-vendored
 * bellman 0.1.0 crate, Cargo.lock:210-212, whose surface as the reference uses it is SURVEY.md 8(b)); "-" = no
 * counterpart in the reference (why it exists is said at the declaration).
 *   zk_params_load, zk_params_free  Parameters::read(reader, checked)             core/proofs/src/confidential.rs:99
 *   zk_params_get_info, zk_params_get_windows   - (fields of Parameters: lengths of the queries; the recoding widths chosen here)
 *   zk_params_get_merged            - (equal points inside the a, b_g1 and b_g2 queries: terms the multiexps do not add twice)
 *   zk_params_get_pairs             - (sums of two bases whose variables tend to hold one value: two terms of a proof as one)
 *   zk_params_write_vk              Parameters.vk, the input of prepare_verifying_key   core/proofs/src/setup.rs:31, 62
 *   zk_prove / zk_prove_batch       create_random_proof -> create_proof           confidential.rs:149, anonymous.rs:165
 *   zk_prove_batch_dev              the same, assignments already in HBM          confidential.rs:149
 *   zk_r1cs_load, zk_r1cs_free      the matrices a Circuit::synthesize enforces   circuit/confidential_transfer.rs:61-305
 *   zk_prove_batch_witness          create_proof; bellman's ProvingAssignment row evaluation
 *   zk_transfer_r1cs_load           structure half of ConfidentialTransfer::synthesize   circuit/confidential_transfer.rs:61-305
 *   zk_transfer_r1cs_fingerprint    TestConstraintSystem::hash / the pinned values       circuit/test.rs:228-251, confidential_transfer.rs:383-386
 *   zk_transfer_witness, zk_transfer_witness_gpu   value half of ConfidentialTransfer::synthesize       circuit/confidential_transfer.rs:29-41, 61-305
 *   zk_transfer_prove_batch         synthesize + create_random_proof              confidential.rs:134-149
 *   zk_pipeline_create, zk_pipeline_submit, zk_pipeline_wait, zk_pipeline_lanes, zk_pipeline_free
 *                                   the same for a stream of batches; - (the reference proves one transaction per call)
 *   zk_spending_key_from_seed       SpendingKey::from_seed                        core/proofs/src/no_std_aliases/keys.rs:45-58
 *   zk_jubjub_base_mul              EncryptionKey::from_decryption_key            no_std_aliases/keys.rs:250-261
 *   zk_elgamal_encrypt              elgamal::Ciphertext::encrypt                  no_std_aliases/elgamal.rs:46-63
 *   zk_elgamal_encrypt_dev          Ciphertext::encrypt / neg_encrypt and MultiCiphertexts::encrypt for groups of keys, in two kernels
 *                                   no_std_aliases/elgamal.rs:46-63, core/proofs/src/crypto_components.rs:60-125, 168-217
 *   zk_elgamal_table_create, zk_elgamal_decrypt, zk_elgamal_table_free
 *                                   elgamal::Ciphertext::decrypt (the brute-force walk) no_std_aliases/elgamal.rs:85-108
 *   zk_elgamal_add                  elgamal::Ciphertext::add / sub                no_std_aliases/elgamal.rs:139-158
 *   zk_confidential_scan, zk_anonymous_scan   - (a block read with one decryption key: Ciphertext::decrypt per value,
 *                                   no_std_aliases/elgamal.rs:85-108, and the signs of MultiCiphertexts::<Anonymous>::encrypt,
 *                                   core/proofs/src/crypto_components.rs:168-220)
 *   zk_scan_keys_create, zk_scan_keys_get, zk_scan_keys_free   - (a set of decryption keys and the encryption key of each:
 *                                   EncryptionKey::from_decryption_key, no_std_aliases/keys.rs:250-261, once per key)
 *   zk_confidential_scan_keys, zk_anonymous_scan_keys   - (a block read with every key of such a set in one call: the parts of the
 *                                   two scans above, keys.rs:250-261, elgamal.rs:85-108, crypto_components.rs:168-220)
 *   zk_balance_keys                 BalanceQuery::get_balance_from_decryption_key for the accounts of a key set in one call
 *                                   zface/src/utils/getter.rs:135-175 (Ciphertext::add, ::write, ::decrypt: elgamal.rs:85-158)
 *   zk_hd_master                    ExtendedSpendingKey::master                   zface/src/derive/mod.rs:48-64
 *   zk_hd_xpgk_from_xsk             From<&ExtendedSpendingKey> for ExtendedProofGenerationKey   zface/src/derive/mod.rs:136-146
 *   zk_hd_derive                    ExtendedSpendingKey::derive_child, ExtendedProofGenerationKey::derive_child for the children of one
 *                                   parent, with into_decryption_key / into_encryption_key of each
 *                                   zface/src/derive/mod.rs:66-104, 164-197, components.rs:15-74, no_std_aliases/keys.rs:166-198
 *   zk_scan_keys_create_hd          - (zk_scan_keys_create for the accounts of such children: zface/src/wallet/keyfile.rs:78-92 per account)
 *   zk_jubjub_base_mul_dev          EncryptionKey::from_decryption_key, ProofGenerationKey::add on the device   no_std_aliases/keys.rs:200-203, 250-261
 *   zk_elgamal_ledger_apply        rollover, sub_enc_balance, add_pending_transfer of a block (Ciphertext::add / sub in order)
 *                                   modules/encrypted-balances/src/lib.rs:133-222, modules/encrypted-assets/src/lib.rs:266-350,
 *                                   modules/anonymous-balances/src/lib.rs:169-225, core/primitives/src/ciphertext.rs:90-100
 *   zk_transfer_derive              the derivations at the head of gen_proof      confidential.rs:105-133
 *   zk_transfer_gen_proof_batch     ProofBuilder::gen_proof (Confidential)        confidential.rs:105-172, check_proof :208-278
 *   zk_anonymous_r1cs_load          structure half of AnonymousTransfer::synthesize      circuit/anonymous_transfer.rs:56-337
 *   zk_anonymous_r1cs_fingerprint   TestConstraintSystem::hash (no pin in the reference) circuit/test.rs:228-251, anonymous_transfer.rs:446-451
 *   zk_anonymous_witness, zk_anonymous_witness_gpu   value half of AnonymousTransfer::synthesize          circuit/anonymous_transfer.rs:40-54, 56-337
 *   zk_anonymous_prove_batch        synthesize + create_random_proof              anonymous.rs:147-165
 *   zk_anonymous_derive             the derivations at the head of gen_proof      anonymous.rs:97-146
 *   zk_anonymous_derive_dev         the same, the point work in two kernels, with check_proof's public inputs   anonymous.rs:97-146, 213-264
 *   zk_r1cs_check_batch, zk_transfer_check_batch, zk_anonymous_check_batch
 *                                   TestConstraintSystem::which_is_unsatisfied / is_satisfied   core/proofs/src/circuit/test.rs:253-272
 *   zk_r1cs_stage                   - (the namespace half of which_is_unsatisfied's answer, circuit/test.rs:253-272: the part of a
 *                                   built-in circuit a constraint index lies in, in this library's own words)
 *   zk_anonymous_gen_proof_batch    ProofBuilder::gen_proof (Anonymous)           anonymous.rs:97-183, check_proof :213-264
 *   zk_generate_parameters          generate_random_parameters                    core/proofs/src/setup.rs:28-31, 59-62
 *   zk_vk_prepare                   prepare_verifying_key                         core/bellman-verifier/src/verifier.rs:15-30
 *   zk_vk_read, zk_vk_write, zk_vk_free   PreparedVerifyingKey::read / write            core/bellman-verifier/src/lib.rs:175-244
 *   zk_vk_num_inputs                pvk.ic.len() - 1                              verifier.rs:38-40
 *   zk_verify_proof / zk_verify_batch   verify_proof                              verifier.rs:32-63; callers confidential.rs:271, modules/zk-system/src/lib.rs:57-108
 *   zk_verify_batch_rlc             - (bellman's batch verifier): the same verdicts, one final exponentiation
 *   zk_proof_read_batch             Proof::read                                   core/bellman-verifier/src/lib.rs:67-110
 *   zk_jubjub_into_xy               IntoXY of the primitives (Point::read + as_prime_order + into_xy)   core/primitives/src/enc_key.rs:89, core/jubjub/src/curve/edwards.rs:92-165, :319-330
 *   zk_confidential_verify_batch    zk_system::verify_confidential_proof          modules/zk-system/src/lib.rs:56-115, input_builder.rs:15-27
 *   zk_anonymous_verify_batch       zk_system::verify_anonymous_proof             modules/zk-system/src/lib.rs:118-165
 *   zk_confidential_block_execute   encrypted_balances::confidential_transfer for every extrinsic of a block, in order
 *                                   modules/encrypted-balances/src/lib.rs:25-96 (rollover :133-170, sub_enc_balance :173-196,
 *                                   add_pending_transfer :199-222), modules/zk-system/src/lib.rs:56-115
 *   zk_anonymous_block_execute      anonymous_balances::anonymous_transfer for every extrinsic of a block, in order
 *                                   modules/anonymous-balances/src/lib.rs:23-82 (rollover :169-206, add_pending_transfer :209-229),
 *                                   modules/zk-system/src/lib.rs:118-165
 *   zk_asset_block_execute          encrypted_assets::issue, confidential_transfer and destroy for every extrinsic of a block, in order
 *                                   modules/encrypted-assets/src/lib.rs:32-83, :86-164, :167-215 (rollover :266-304, sub_enc_balance
 *                                   :307-331, add_pending_transfer :334-358), modules/zk-system/src/lib.rs:56-115
 *   zk_g_epoch                      GEpoch::group_hash                       core/primitives/src/g_epoch.rs:102-110, core/jubjub/src/group_hash.rs:17-46
 *   zk_redjubjub_sign               redjubjub::PrivateKey::sign                 core/jubjub/src/redjubjub.rs:73-103; callers confidential.rs:416-420, anonymous.rs:378-401
 *   zk_redjubjub_verify_batch       redjubjub::PublicKey::verify, per signature   core/jubjub/src/redjubjub.rs:127-155; RedjubjubSignature::verify core/primitives/src/signature.rs:65-82
 *   zk_msm_create, zk_msm_create_variable, zk_msm_run, zk_msm_run_dev, zk_msm_free, zk_msm_g1, zk_msm_g2, zk_msm_cache_release
 *                                   bellman multiexp(FullDensity); group law core/pairing/src/bls12_381/ec.rs:296-526
 *   zk_ntt_fr, zk_ntt_create, zk_ntt_run_dev, zk_ntt_free
 *                                   bellman EvaluationDomain {fft, ifft, coset_fft, icoset_fft}; field core/pairing/src/bls12_381/fr.rs:341-571
 *   zk_debug_field_mul              Fr / Fq mul_assign (for the literal KATs)     fr.rs:438-464, fq.rs:915-965
 *   zk_strerror / zk_last_error     the variants of SynthesisError and their texts   core/bellman-verifier/src/lib.rs:359-383
 *   zk_device_count, zk_set_host_threads, zk_bind_host_to_device, zk_stream, zk_synchronize, zk_kernel_forms, zk_memory_stats,
 *   zk_profile_begin, zk_profile_get, zk_profile_end   - (device selection, host threads, measurement; the reference runs on the CPU)
 */
#ifndef ZKAMD_H
#define ZKAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t zk_status;

enum {
    ZK_OK = 0,
    ZK_ERR_ASSIGNMENT_MISSING = 1,          /* SynthesisError::AssignmentMissing */
    ZK_ERR_DIVISION_BY_ZERO = 2,            /* SynthesisError::DivisionByZero */
    ZK_ERR_UNSATISFIABLE = 3,               /* SynthesisError::Unsatisfiable */
    ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE = 4, /* SynthesisError::PolynomialDegreeTooLarge */
    ZK_ERR_UNEXPECTED_IDENTITY = 5,         /* SynthesisError::UnexpectedIdentity */
    ZK_ERR_IO = 6,                          /* SynthesisError::IoError (malformed / short pk) */
    ZK_ERR_MALFORMED_VERIFYING_KEY = 7,     /* SynthesisError::MalformedVerifyingKey */
    ZK_ERR_UNCONSTRAINED_VARIABLE = 8,      /* SynthesisError::UnconstrainedVariable */
    ZK_ERR_INVALID_ARGUMENT = 16,
    ZK_ERR_DEVICE = 17,                     /* HIP runtime error; see zk_last_error() */
    ZK_ERR_NO_DEVICE = 18,
    ZK_ERR_OUT_OF_MEMORY = 19
};

#define ZK_FR_MONTGOMERY 1u /* flag: scalars are raw Montgomery-form Fr limbs */

const char* zk_strerror(zk_status st);
/* Human-readable detail of the last failure on this thread (HIP error string, offending index). */
const char* zk_last_error(void);
zk_status zk_device_count(int* count);
/* Host threads the library may use for its CPU-side legs (witness calculation of zk_transfer_*,
 * proof encoding).  0 = default: ZKAMD_HOST_THREADS, else the cores of the process's affinity mask.
 * One process per GPU on a multi-GPU node should pass cores / ranks. */
void zk_set_host_threads(int n);

/* One process per GPU: restrict the CALLING thread - and every thread it starts afterwards, the
 * library's workers included - to the CPUs of the NUMA node the GPU hangs off (hipDeviceGetPCIBusId ->
 * /sys/bus/pci/devices/<id>/numa_node -> /sys/devices/system/node/node<N>/cpulist, intersected with the mask the
 * process was given).  Call it first, before zk_params_load / zk_pipeline_create.  *numa_node_out = the node, or -1
 * when the platform reports none or its CPUs are not ours (the mask is then left as it was); *n_cpus_out = CPUs the
 * thread may run on afterwards.  No reference counterpart: the reference proves on the CPU in one process
 * (core/proofs/src/confidential.rs:149). */
zk_status zk_bind_host_to_device(int device, int* numa_node_out, int* n_cpus_out);

/* ------------------------------------------------------------------------------------------
 * Parameters  (bellman groth16::Parameters<Bls12>)
 * replaces: Parameters::read(reader, checked)   reference call: confidential.rs:99
 * Byte format (bellman Parameters::write): vk = alpha_g1 | beta_g1 | beta_g2 |
 * gamma_g2 | delta_g1 | delta_g2 | u32be n_ic | ic[] ; then u32be len | points for h, l, a,
 * b_g1 (G1) and b_g2 (G2).  checked != 0 additionally verifies on-curve and subgroup membership
 * of every point (on the GPU); both modes reject the point at infinity, as bellman does.
 * The bases are uploaded once, expanded into the table of all their doublings 2^k * P (k = 0..254;
 * ~4.2 GB for the transfer key) and stay resident in HBM.
 * ------------------------------------------------------------------------------------------ */
typedef struct zk_params zk_params;

typedef struct {
    uint32_t n_ic, n_h, n_l, n_a, n_b_g1, n_b_g2;
    uint32_t log_domain;  /* m = 2^log_domain = n_h + 1 */
    uint32_t window_bits; /* width c of the NAF recoding used for the G1 jobs of this key */
    uint32_t n_windows;   /* table slices per base (255: every doubling 2^k * P) */
    uint32_t device;
    uint64_t device_bytes; /* HBM held by the handle (tables + twiddles) */
} zk_params_info;

zk_status zk_params_load(const uint8_t* pk_bytes, size_t len, int checked, int device, zk_params** out);
zk_status zk_params_get_info(const zk_params* p, zk_params_info* info);
/* The recoding widths in use: out[0] = the C' jobs (H + L + r B1) of a batch, out[1] = its A jobs, out[2] = both G1 jobs
 * of a few proofs made alone (one launch set), out[3] = the G2 job (B2).  zk_params_info.window_bits is out[0]. */
zk_status zk_params_get_windows(const zk_params* p, uint32_t out[4]);
/* Entries minus distinct points of the a, b_g1 and b_g2 queries (out[0..2]): variables with identical QAP columns have
 * equal points, which a proof's multiexps take as one term under the sum of their scalars. */
zk_status zk_params_get_merged(const zk_params* p, uint32_t out[3]);
/* Value pairs of the key and the circuit it was last bound to by a statement-to-proof entry (all zero before that, and for a
 * circuit the library has no probe statements for): out[0..3] = the bases P_j + P_p kept for the a, b_g1, b_g2 and l
 * queries, one per linked pair of variables that has both terms in the query; out[4..7] = the terms a proof is expected to
 * merge in each of them (the mean over the library's probe statements).  Two linked variables that hold the same value in
 * a proof are one term of its multiexps over the sum of their bases; ZKAMD_MERGE_VALUES=0 keeps a term per variable. */
zk_status zk_params_get_pairs(const zk_params* p, uint32_t out[8]);
void zk_params_free(zk_params* p);

/* ------------------------------------------------------------------------------------------
 * Proving  (bellman groth16::create_proof(circuit, params, r, s) after synthesis)
 * replaces: create_random_proof / create_proof   reference call: confidential.rs:149
 * The assignment is exactly bellman's ProvingAssignment after `circuit.synthesize` and the
 * per-input `Input(i) * 0 = 0` rows: the row evaluations a, b, c (n_rows each), the input and
 * aux assignments, and the three density trackers (one byte per variable, 0 / 1).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t n_rows;   /* constraints + n_inputs */
    uint32_t n_inputs; /* including ONE */
    uint32_t n_aux;
    uint32_t flags;    /* ZK_FR_MONTGOMERY */
    const uint8_t* a;  /* n_rows x 32 */
    const uint8_t* b;
    const uint8_t* c;
    const uint8_t* inputs;          /* n_inputs x 32 */
    const uint8_t* aux;             /* n_aux x 32 */
    const uint8_t* a_aux_density;   /* n_aux bytes */
    const uint8_t* b_input_density; /* n_inputs bytes */
    const uint8_t* b_aux_density;   /* n_aux bytes */
} zk_assignment;

/* r, s: 32-byte little-endian PLAIN scalars (the two Fr::rand draws of create_random_proof). */
zk_status zk_prove(zk_params* p, const zk_assignment* asg, const uint8_t r[32], const uint8_t s[32],
                   uint8_t proof_out[192]);

/* n independent proofs of the same circuit (same shape and densities).  rs: n x 64 bytes
 * (r then s per proof).  proofs_out: n x 192 bytes. */
zk_status zk_prove_batch(zk_params* p, size_t n, const zk_assignment* asgs, const uint8_t* rs,
                         uint8_t* proofs_out);

/* Same, with the assignments already resident in HBM (device pointers, plain scalars unless
 * ZK_FR_MONTGOMERY): a, b, c are [n][n_rows][32]; wit is [n][n_inputs + n_aux][32];
 * rs is a HOST pointer.  Densities are host byte arrays shared by the whole batch. */
typedef struct {
    uint32_t n_rows, n_inputs, n_aux, flags;
    const void* d_a;
    const void* d_b;
    const void* d_c;
    const void* d_wit;
    const uint8_t* a_aux_density;
    const uint8_t* b_input_density;
    const uint8_t* b_aux_density;
} zk_batch_dev;
zk_status zk_prove_batch_dev(zk_params* p, size_t n, const zk_batch_dev* batch, const uint8_t* rs,
                             uint8_t* proofs_out);

/* ------------------------------------------------------------------------------------------
 * Proving from the variable assignment alone (row f-1 of the hot-path scope).
 * bellman's ProvingAssignment evaluates every constraint row on the host while the circuit is
 * synthesized (a_j = <A_j, z>, b_j, c_j).  The R1CS of a circuit is fixed,
 * so it can live on the GPU: zk_r1cs_load takes the three matrices in CSR form once, and
 * zk_prove_batch_witness takes only z = (inputs | aux) per proof - a quarter of the bytes - and
 * computes a, b, c with a sparse matrix-vector product on the device.  The density trackers and
 * the per-input rows `Input(i) * 0 = 0` are derived from the matrices exactly as bellman's prover
 * derives them.  Coefficients: 32 bytes little-endian plain integers < r.
 * ------------------------------------------------------------------------------------------ */
typedef struct zk_r1cs zk_r1cs;
typedef struct {
    const uint32_t* row_ptr; /* n_constraints + 1 */
    const uint32_t* col;     /* variable index: input i -> i, aux j -> n_inputs + j */
    const uint8_t* coeff;    /* nnz x 32 */
} zk_csr;
zk_status zk_r1cs_load(uint32_t n_inputs, uint32_t n_aux, uint32_t n_constraints, const zk_csr* a, const zk_csr* b,
                       const zk_csr* c, int device, zk_r1cs** out);
void zk_r1cs_free(zk_r1cs* r);
/* The constraint system of the reference's confidential-transfer circuit, emitted natively by the library (the
 * structure half of ConfidentialTransfer::synthesize, core/proofs/src/circuit/confidential_transfer.rs:61-305):
 * zk_transfer_r1cs_load = zk_r1cs_load of those matrices.  zk_transfer_r1cs_fingerprint returns the counts and
 * the blake2s hash of the normalised system as the reference's circuit test defines it
 * (core/proofs/src/circuit/test.rs:228-251); the reference pins 19 974 constraints, 23 inputs and
 * d23c92fb60ee547d45118e160679929cfa186957280673af62f09fa12d401784 (confidential_transfer.rs:383-386). */
zk_status zk_transfer_r1cs_load(int device, zk_r1cs** out);
zk_status zk_transfer_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints);
/* witness: n x (n_inputs + n_aux) x 32 bytes on the HOST (plain, or Montgomery limbs with
 * ZK_FR_MONTGOMERY in flags); rs: n x 64; proofs_out: n x 192. */
zk_status zk_prove_batch_witness(zk_params* p, zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags,
                                 const uint8_t* rs, uint8_t* proofs_out);

/* ------------------------------------------------------------------------------------------
 * Native witness calculator of the reference's confidential-transfer circuit (row a3 / f-1).
 * replaces, value-wise: ConfidentialTransfer::synthesize under bellman's ProvingAssignment
 *   core/proofs/src/circuit/confidential_transfer.rs:61-305 (+ range_check.rs, utils.rs and the
 *   sapling-crypto gadgets).  The statement is the ten private values of the circuit
 *   (confidential_transfer.rs:29-41): u32 amounts, Fs scalars as 32 bytes little-endian, Jubjub
 *   points in the reference's 32-byte encoding (core/jubjub/src/curve/edwards.rs:92-117, 190-206).
 * zk_transfer_witness writes z = (23 inputs | 19 955 aux) per statement, in the reference's
 * variable order (host, multithreaded); zk_transfer_prove_batch = witness + row evaluations on
 * the GPU + create_proof, for the R1CS loaded with zk_r1cs_load.
 * ------------------------------------------------------------------------------------------ */
#define ZK_TRANSFER_N_INPUTS 23u
#define ZK_TRANSFER_N_AUX 19955u
typedef struct {
    uint32_t amount, remaining_balance, fee, reserved;
    uint8_t randomness[32], alpha[32], dec_key_sender[32];
    uint8_t proof_generation_key[32], enc_key_recipient[32], enc_balance_left[32], enc_balance_right[32], g_epoch[32];
} zk_transfer_statement;
/* witness_out: n x (23 + 19955) x 32 bytes; plain little-endian, or Montgomery limbs with ZK_FR_MONTGOMERY */
zk_status zk_transfer_witness(const zk_transfer_statement* st, size_t n, uint32_t flags, uint8_t* witness_out);
zk_status zk_transfer_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_transfer_statement* st,
                                  const uint8_t* rs, uint8_t* proofs_out);
/* zk_transfer_prove_batch and zk_pipeline compute the witnesses ON THE GPU (one thread per statement and gadget,
 * the assignment never leaves HBM) - except for a handful of statements (n <= 8 x host threads: one transaction at a time,
 * the reference's call pattern), whose assignments the native host calculator computes faster than the kernels' 8.4 ms of
 * serial chains; ZKAMD_WITNESS = host | gpu forces an engine, the proof bytes do not depend on it.  This entry returns
 * what that generator produces - same format as zk_transfer_witness - so that the two can be compared. */
zk_status zk_transfer_witness_gpu(zk_r1cs* circuit, const zk_transfer_statement* st, size_t n, uint32_t flags,
                                  uint8_t* witness_out);

/* A stream of statement batches: submit() queues a batch and returns at once; worker threads (one per lane, two lanes
 * by default) enqueue the witness kernels of a chunk beside the proving of the chunk before it, so two chunks are in flight
 * (ZKAMD_WITNESS=host: one lane, whose helper thread computes the witnesses of the next chunk on the host cores,
 * zk_set_host_threads, into the circuit handle's page-locked buffer while the lane proves the current one);
 * wait() blocks until everything submitted so far is proved and returns the first failure, if any (the
 * statement index in its message is relative to the failing submit).  The caller's buffers (statements, rs,
 * proofs_out) must stay valid until wait() returns, and `p` / `circuit` must not be used by other calls
 * while batches are in flight.  Batches larger than a device chunk (1024) are cut into chunks. */
typedef struct zk_pipeline zk_pipeline;
zk_status zk_pipeline_create(zk_params* p, zk_r1cs* circuit, zk_pipeline** out);
zk_status zk_pipeline_submit(zk_pipeline* pl, size_t n, const zk_transfer_statement* st, const uint8_t* rs,
                             uint8_t* proofs_out);
zk_status zk_pipeline_wait(zk_pipeline* pl);
/* chunks proved concurrently (ZKAMD_PIPELINE_LANES, default 2; fewer when the device's free memory does not hold the
 * workspaces of that many lanes - about 36 MB per proof of a chunk and lane) */
int zk_pipeline_lanes(const zk_pipeline* pl);
void zk_pipeline_free(zk_pipeline* pl);

/* ------------------------------------------------------------------------------------------
 * gen_proof: the reference's wallet-level entry (ProofBuilder::gen_proof, core/proofs/src/confidential.rs:
 * 105-172) for a batch of transfers.  Per request: the proof generation key G * sk, the decryption key
 * Blake2s("zech_bdk", pgk) with its five top bits dropped and the sender's encryption key
 * (no_std_aliases/keys.rs:132-198), rvk = pgk + alpha G, nonce = dec_key * g_epoch, the proof, the ElGamal
 * ciphertexts of amount and fee under both keys (elgamal.rs:46-63), check_proof against the prepared verifying key
 * (confidential.rs:208-278; ZK_ERR_UNSATISFIABLE if a proof does not verify, as the reference) and the packing of
 * ConfidentialXt (gen_xt :282-354, the struct :358-370), rsk = sk + alpha.  randomness / alpha are the two Fs::rand draws of gen_proof,
 * rs (n x 64 bytes) the two Fr::rand draws of create_random_proof; scalars 32 bytes little-endian, points in the
 * 32-byte Jubjub encoding.
 * zk_transfer_derive is the host half alone (request -> statement and rsk); zk_spending_key_from_seed is
 * SpendingKey::from_seed (keys.rs:45-58).  The points of a REQUEST (recipient key, encrypted balance, g_epoch) pass
 * through as_prime_order as the reference's typed readers do (keys.rs:269-276, elgamal.rs:117-133): a point outside the
 * prime-order subgroup is ZK_ERR_INVALID_ARGUMENT.  The points of a STATEMENT (zk_transfer_statement, the circuit
 * instance itself, whose fields are Point<E, PrimeOrder> by type in the reference) are decoded and curve-checked only.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t amount, fee, remaining_balance, reserved;
    uint8_t spending_key[32];
    uint8_t enc_key_recipient[32], enc_balance_left[32], enc_balance_right[32], g_epoch[32];
    uint8_t randomness[32], alpha[32];
} zk_transfer_request;
typedef struct {   /* ConfidentialXt, confidential.rs:358-370 */
    uint8_t proof[192];
    uint8_t enc_key_sender[32], enc_key_recipient[32], left_amount_sender[32], left_amount_recipient[32], left_fee[32],
        right_randomness[32], rsk[32], rvk[32], enc_balance[64], nonce[32];
} zk_confidential_xt;
zk_status zk_spending_key_from_seed(const uint8_t* seed, size_t len, uint8_t spending_key_out[32]);
/* The two Jubjub operations every key and ciphertext a wallet hands to gen_proof is made of (so a batch of requests can
 * be built without the reference's host code):
 * zk_jubjub_base_mul: scalar * FixedGenerators::NoteCommitmentRandomness, the generator of the reference's keys and
 *   ciphertexts; with the decryption key this is EncryptionKey::from_decryption_key (no_std_aliases/keys.rs:250-261).
 *   scalars: n x 32 bytes little-endian canonical Fs; points_out: n x 32 bytes (edwards::Point::write).
 * zk_elgamal_encrypt: elgamal::Ciphertext::encrypt (no_std_aliases/elgamal.rs:46-63): left = value G + randomness
 *   enc_key, right = randomness G.  enc_keys pass through as_prime_order as EncryptionKey::read does (keys.rs:269-276). */
zk_status zk_jubjub_base_mul(const uint8_t* scalars, size_t n, uint8_t* points_out);
zk_status zk_elgamal_encrypt(const uint32_t* values, const uint8_t* randomness, const uint8_t* enc_keys, size_t n,
                             uint8_t* left_out, uint8_t* right_out);
/* zk_elgamal_encrypt_dev: the same encryption for n GROUPS of k keys as a stage on `device` (csrc/elgamal_encrypt.h).  Group i has
 *   one randomness r_i: right_i = [r_i]G, left_ij = [v_ij]G + [r_i]pk_ij, G the generator of zk_elgamal_encrypt.
 *   k = 1 with v >= 0 is Ciphertext::encrypt; a negative value is Ciphertext::neg_encrypt (crypto_components.rs:181-187); k = 3 with
 *   (amount, amount, fee) under (sender, recipient, sender) is MultiCiphertexts::<Confidential>::encrypt (crypto_components.rs:60-125);
 *   k = 12 with -amount at the sender, +amount at the recipient and 0 elsewhere is the anonymous one (:168-217).
 *   values: n x k, |v| < 2^32; randomness: n x 32 bytes, canonical Fs, little-endian; enc_keys: n x k x 32 bytes.
 *   Outputs: left_out n x k x 32 and right_out n x 32 bytes, Point::write of the affine result (the identity is 01 00 .. 00);
 *   status_out: n x k bytes.  Keys pass Point::read and as_prime_order, exactly as zk_jubjub_into_xy decides: status_out[i k + j]
 *   is 0 or the ZK_INTO_XY_* code of that key.  A refused key is a status, never an error: it zeroes its own 32 bytes of left_out
 *   and touches nothing else - right_i and the other lefts of its group are written as usual.
 *   ZK_ERR_INVALID_ARGUMENT, nothing written, the index in zk_last_error: k outside 1 .. 16, a value outside (-2^32, 2^32), a
 *   randomness that is not canonical, a NULL pointer with n > 0.  n == 0 touches nothing.
 *   Two forms that write the same bytes: host threads for device < 0 or n k <= ZKAMD_ENCRYPT_HOST_MAX (README), else two kernels
 *   per slice of 4096 groups on `device` - every distinct key decoded once, [r_i]G once per group.  The randomness is the
 *   sender's secret: every device buffer that held it is zeroed before the call returns.  The device form is not constant-time. */
zk_status zk_elgamal_encrypt_dev(size_t n, size_t k, const int64_t* values, const uint8_t* randomness, const uint8_t* enc_keys,
                                 int device, uint8_t* left_out, uint8_t* right_out, uint8_t* status_out);
zk_status zk_transfer_derive(const zk_transfer_request* req, size_t n, zk_transfer_statement* statements_out, uint8_t* rsk_out);
/* The balance query at the head of a transfer (zface/src/utils/getter.rs:135-174): the encrypted balance and the pending
 * transfer are added (zk_elgamal_add) and the sum is decrypted (zk_elgamal_decrypt).
 * zk_elgamal_table_create: the baby steps { j G : j < 2^baby_bits } of a discrete-log search, built on `device` and kept there
 *   (G = FixedGenerators::NoteCommitmentRandomness, the generator of zk_elgamal_encrypt; zface's getter calls the same index-1
 *   generator Diversifier).  baby_bits 8 .. 24, 0 = 20: 64 MB of coordinates and 16 MB of hash slots.  Create one per
 *   wallet process.
 * zk_elgamal_decrypt: elgamal::Ciphertext::decrypt (no_std_aliases/elgamal.rs:85-108) for n ciphertexts (left, right: n x 32
 *   bytes each): found_out[i] = 1 and values_out[i] = x exactly when x G == left - dk right and x < limit, else both 0 (the
 *   reference's None).  limit = ZK_ELGAMAL_DECRYPT_LIMIT is the reference's bound; any limit 1 .. 2^32 is searched, 2^32
 *   decrypts every u32 amount.  dec_keys: canonical Fs scalars, 32 bytes little-endian; dec_key_stride 0 = one key for all,
 *   32 = one key per ciphertext.  Both points pass through as_prime_order as Ciphertext::read does (elgamal.rs:116-133).
 *   left - dk right is computed on host threads; the search (one probe per ciphertext for limit <= 2^baby_bits, else
 *   ceil(limit / 2^baby_bits) giant steps) runs on the table's device.
 * zk_elgamal_add: Ciphertext::add, or Ciphertext::sub with subtract != 0 (elgamal.rs:139-158), for n pairs; host only.
 * A refusal fails the whole call with ZK_ERR_INVALID_ARGUMENT naming the index and the field. */
#define ZK_ELGAMAL_DECRYPT_LIMIT 1000000u   /* the reference's bound, elgamal.rs:100 */
typedef struct zk_elgamal_table zk_elgamal_table;
zk_status zk_elgamal_table_create(uint32_t baby_bits, int device, zk_elgamal_table** out);
zk_status zk_elgamal_decrypt(zk_elgamal_table* t, size_t n, const uint8_t* left, const uint8_t* right, const uint8_t* dec_keys,
                             size_t dec_key_stride, uint64_t limit, uint32_t* values_out, uint8_t* found_out);
void zk_elgamal_table_free(zk_elgamal_table* t);
zk_status zk_elgamal_add(const uint8_t* left_a, const uint8_t* right_a, const uint8_t* left_b, const uint8_t* right_b, size_t n,
                         int subtract, uint8_t* left_out, uint8_t* right_out);
/* Reading a block with ONE decryption key: which of n accepted extrinsics touch the wallet's key, and by how much.  The reference
 * has no counterpart (zface reads one balance, getter.rs:135-174, and keeps no history); the parts are its own: the key is
 * EncryptionKey::from_decryption_key(dec_key) (no_std_aliases/keys.rs:250-261, computed once per call), its 32 canonical bytes
 * are compared with the keys an extrinsic carries, and every value is Ciphertext::decrypt (elgamal.rs:85-108) over [0, limit),
 * limit 1 .. 2^32, with the search of zk_elgamal_decrypt on the table's device.  dec_key: a canonical Fs scalar, else
 * ZK_ERR_INVALID_ARGUMENT; taking the decryption key alone, a caller cannot hand over a pair that does not belong together.
 * zk_confidential_scan: role bit ZK_SCAN_SENDER when enc_key_sender is the wallet's, ZK_SCAN_RECIPIENT when enc_key_recipient
 *   is (3: a transfer to oneself, 0: neither, and nothing else of that xt is looked at).  The sender decrypts
 *   (left_amount_sender, right_randomness) into amount_sent and (left_fee, right_randomness) into fee, the recipient
 *   (left_amount_recipient, right_randomness) into amount_received (confidential.rs:150-157: one right half for all three).
 *   A value that is not below the limit - or was encrypted under another key - leaves its found bit clear and its field 0.
 * zk_anonymous_scan: members has bit i set when enc_keys[i] is the wallet's (a key may appear more than once).  For each such
 *   i the value of v = left_ciphertexts[i] - dec_key * right_ciphertext is x < limit with x G == v, or -x with x G == -v:
 *   MultiCiphertexts::<Anonymous>::encrypt (crypto_components.rs:168-220) puts -amount under the sender's key, +amount under
 *   the recipient's and 0 under every decoy's.  delta is the sum over the occurrences - what the ledger adds to this key's
 *   balance (modules/anonymous-balances/src/lib.rs:169-225) - and found 1 only when every occurrence has a value; else delta is 0.
 * Refusals are results, never errors.  Only the points the wallet's role uses are read, as Ciphertext::read reads them
 *   (Point::read, then as_prime_order: what zk_jubjub_into_xy decides): refusal = (field number of zk_confidential_verify_batch /
 *   zk_anonymous_verify_batch) | (ZK_INTO_XY_* status << 6) of the first of them, in push order, that is refused; found and the
 *   values of that extrinsic are then 0.  A malformed point in an extrinsic that does not match is not looked at.
 * NOT looked at: proofs, signatures, rvk, rsk, nonce and enc_balance.  The scan is for extrinsics the chain has ACCEPTED (verify
 *   them with zk_confidential_verify_batch / zk_anonymous_verify_batch and zk_redjubjub_verify_batch first).
 * Up to ZKAMD_SCAN_HOST_MAX values to decrypt (default 128, the measured crossover on 16 host threads; read per
 *   call; 0 = always the kernels) the point work - decoding, dec_key * right once per extrinsic - runs on the host threads, above it in two
 *   kernels on the table's device (csrc/elgamal_scan.h); the bytes written do not depend on the form.  dec_key and everything
 *   derived from it are wiped on the host and zeroed on the device before the call returns.  The host form multiplies without
 *   branching on dec_key; the device form is NOT constant-time: the recoded digits of dec_key decide where its chain adds.
 * t == NULL, or a NULL xts / dec_key / out with n > 0: ZK_ERR_INVALID_ARGUMENT.  n == 0 touches nothing. */
enum { ZK_SCAN_SENDER = 1, ZK_SCAN_RECIPIENT = 2 };                       /* role bits */
enum { ZK_SCAN_FOUND_SENT = 1, ZK_SCAN_FOUND_FEE = 2, ZK_SCAN_FOUND_RECEIVED = 4 };
typedef struct {            /* 16 bytes */
    uint8_t role;           /* 0: neither key of the xt is the wallet's; 3: a transfer to oneself */
    uint8_t found;          /* which of the three values below were found below the limit */
    uint8_t refusal;        /* 0, or field | status << 6 */
    uint8_t reserved;       /* 0 */
    uint32_t amount_sent, fee, amount_received;
} zk_confidential_scan_result;
typedef struct {            /* 16 bytes */
    uint16_t members;       /* bit i set: enc_keys[i] is the wallet's key; 0: absent */
    uint8_t found;          /* 1: every occurrence decrypted to a value with |value| < limit */
    uint8_t refusal;        /* 0, or field | status << 6 */
    uint32_t reserved;      /* 0 */
    int64_t delta;          /* sum over the occurrences: +a received, -a sent, 0 decoy */
} zk_anonymous_scan_result;
/* zk_elgamal_ledger_apply: what the three balance modules do to storage around every proof of a block (rollover,
 *   sub_enc_balance, add_pending_transfer: modules/encrypted-balances/src/lib.rs:133-222, modules/encrypted-assets/src/lib.rs:266-350;
 *   twelve updates per extrinsic in modules/anonymous-balances/src/lib.rs:169-225) - Ciphertext::add / Ciphertext::sub
 *   (core/primitives/src/ciphertext.rs:90-100) applied to n_slots stored ciphertexts one op after another, in index order.
 *   INTEGRATION.md, "A block's balance updates", maps the modules' calls to slots and ops.
 *   Reading: every ciphertext, of a slot or of an op, is read as elgamal::Ciphertext::read does - both points through Point::read
 *     and as_prime_order, exactly what zk_jubjub_into_xy decides (x = 0 with the sign bit set is accepted, as there).
 *   op_status_out[i]: 0, or (1 = left, 2 = right) | (IntoXY status << 6) of the first point of op i that is refused - the
 *     refusal_out convention of zk_confidential_verify_batch; slot_status_out[s] the same for slot s.  A refusal is a status,
 *     never an error.
 *   before_out[i] (may be NULL): the value of slot ops[i].slot just before op i, also for a refused or skipped op.
 *   An op that is neither refused nor skipped (flags bit 1) adds its ciphertext to its slot, or subtracts it (flags bit 0);
 *     slots_out[s] is the value after the last op.  For a refused slot slots_out[s] and the before_out of all its ops are 64
 *     zero bytes; those ops keep their own statuses.
 *   Outputs are Point::write of the affine result (the identity is 01 00 .. 00): canonical, the same bytes in either form.
 *   ops[i].slot >= n_slots, an unknown flag bit or a NULL required pointer with a non-zero count: ZK_ERR_INVALID_ARGUMENT naming
 *     the index, nothing written.  n_ops == 0 copies the judged slots through; with both counts 0 no buffer is touched.
 *   device < 0, or 2 (n_slots + n_ops) <= ZKAMD_INTO_XY_HOST_MAX points: on host threads; else on `device`.
 *   The skip bit is for two passes over a block: the first, with before_out, yields the enc_balances of
 *   zk_confidential_verify_batch; the second, with skip set on the extrinsics that were rejected, the state to store.
 *   The data is public chain state: nothing here is constant-time, and no buffer is wiped. */
#define ZK_LEDGER_SUBTRACT 1u
#define ZK_LEDGER_SKIP 2u
typedef struct {
    uint32_t slot;    /* index into slots */
    uint32_t flags;   /* bit 0: subtract (Ciphertext::sub); bit 1: skip - read and judged, not applied */
    uint8_t left[32], right[32];
} zk_ledger_op;
zk_status zk_elgamal_ledger_apply(size_t n_slots, const uint8_t* slots /* n_slots x 64: left | right */,
                                  size_t n_ops, const zk_ledger_op* ops, int device,
                                  uint8_t* slots_out /* n_slots x 64 */, uint8_t* before_out /* n_ops x 64, may be NULL */,
                                  uint8_t* slot_status_out /* n_slots */, uint8_t* op_status_out /* n_ops */);
struct zk_vk;
zk_status zk_transfer_gen_proof_batch(zk_params* p, zk_r1cs* circuit, struct zk_vk* vk, size_t n, const zk_transfer_request* req,
                                      const uint8_t* rs, zk_confidential_xt* out);

/* The value half of AnonymousTransfer::synthesize (core/proofs/src/circuit/anonymous_transfer.rs:56-337,
 * anonimity_set.rs; ANONIMITY_SIZE = 12, constants.rs:1): the private values of the instance (:40-54) ->
 * the variable assignment bellman's ProvingAssignment would hold, [105 inputs | 50429 aux].  Scalars are
 * FsRepr::write_le bytes, points edwards::Point::write bytes; member i of the anonymity set owns
 * enc_keys[i], left_ciphertexts[i] and its encrypted balance (left, right).  Prove with
 * zk_prove_batch_witness over the circuit's matrices (zk_anonymous_r1cs_load). */
#define ZK_ANONYMOUS_SIZE 12
#define ZK_ANONYMOUS_N_INPUTS 105
#define ZK_ANONYMOUS_N_AUX 50429
typedef struct {
    uint32_t amount, remaining_balance, s_index, t_index;
    uint8_t randomness[32], alpha[32], dec_key[32];
    uint8_t proof_generation_key[32], g_epoch[32];
    uint8_t enc_keys[ZK_ANONYMOUS_SIZE][32], left_ciphertexts[ZK_ANONYMOUS_SIZE][32];
    uint8_t enc_balances_left[ZK_ANONYMOUS_SIZE][32], enc_balances_right[ZK_ANONYMOUS_SIZE][32];
} zk_anonymous_statement;
/* witness_out: n x (105 + 50429) x 32 bytes; plain little-endian, or Montgomery limbs with ZK_FR_MONTGOMERY */
zk_status zk_anonymous_witness(const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* witness_out);
/* The same vectors from the GPU witness generator (csrc/witness_anon_gpu.h; tests compare the two element by element) */
zk_status zk_anonymous_witness_gpu(zk_r1cs* circuit, const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* witness_out);
/* statement -> proof for that circuit (create_random_proof of AnonymousTransfer, core/proofs/src/anonymous.rs:165):
 * witness generation on the GPU (round 4; a handful of statements, or ZKAMD_WITNESS=host: the host calculator), the kernels of
 * chunk k + 1 beside row evaluations + create_proof of chunk k, over the matrices loaded with zk_anonymous_r1cs_load. */
zk_status zk_anonymous_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_anonymous_statement* st,
                                   const uint8_t* rs, uint8_t* proofs_out);
/* The constraint system of that circuit, emitted natively (the structure half of AnonymousTransfer::synthesize):
 * zk_anonymous_r1cs_load = zk_r1cs_load of its matrices; the fingerprint is defined as for the transfer circuit
 * (core/proofs/src/circuit/test.rs:228-251).  The reference holds NO pin for it: the figures next to its test
 * (anonymous_transfer.rs:446-451: 50 634 constraints, 625c4b5d...ea37) are commented out and stale against the
 * source beside them, which has 50 514 constraints. */
zk_status zk_anonymous_r1cs_load(int device, zk_r1cs** out);
zk_status zk_anonymous_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints);

/* ------------------------------------------------------------------------------------------
 * Which constraint an assignment breaks, checked on the GPU before anything is proved.
 * replaces: TestConstraintSystem::which_is_unsatisfied / is_satisfied (core/proofs/src/circuit/test.rs:253-272).
 * The proving entries turn an assignment that satisfies nothing into 192 bytes that do not verify; these entries say
 * beforehand, per assignment, whether a_j * b_j = c_j holds for every constraint j of the loaded matrices, and where it
 * does not - with no key, no transform and no multiexp (csrc/r1cs_check.h).
 *   first_bad  the lowest j with a_j * b_j != c_j, or ZK_R1CS_SATISFIED
 *   n_bad      how many such j
 *   flags      ZK_R1CS_ONE_IS_NOT_ONE: input 0 of the assignment is not 1 (such a vector may satisfy every row and
 *              still does not verify: ONE is an input like any other)
 * A verdict is not an error: an unsatisfied assignment returns ZK_OK with its verdict filled in.  n = 0 writes nothing.
 * zk_r1cs_check_batch: any loaded system; witness as for zk_prove_batch_witness (n x (n_inputs + n_aux) x 32 bytes, plain
 * or ZK_FR_MONTGOMERY; a scalar >= r is ZK_ERR_INVALID_ARGUMENT), in the same chunks.  zk_transfer_check_batch /
 * zk_anonymous_check_batch: the statements of the built-in circuits, through the witness engine the prove entries would
 * pick (ZKAMD_WITNESS) and with their refusals of a malformed statement.  out: n verdicts.
 * zk_r1cs_stage names the part of a built-in circuit a constraint lies in ("range: amount", "balance equation", ...):
 * *stage_out = its number in the circuit's order, [*first_out, *first_out + *count_out) its constraints, name_out its
 * name (cut to name_cap - 1 characters, always terminated); every out pointer may be null.  Matrices loaded with
 * zk_r1cs_load carry no table: *stage_out = 0xFFFFFFFF, the whole system as the range and an empty name.  A constraint
 * >= n_constraints is ZK_ERR_INVALID_ARGUMENT.
 * ------------------------------------------------------------------------------------------ */
#define ZK_R1CS_SATISFIED 0xFFFFFFFFu
#define ZK_R1CS_ONE_IS_NOT_ONE 1u
typedef struct {
    uint32_t first_bad, n_bad, flags, reserved;
} zk_r1cs_verdict;
zk_status zk_r1cs_check_batch(zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags, zk_r1cs_verdict* out);
zk_status zk_transfer_check_batch(zk_r1cs* circuit, size_t n, const zk_transfer_statement* st, zk_r1cs_verdict* out);
zk_status zk_anonymous_check_batch(zk_r1cs* circuit, size_t n, const zk_anonymous_statement* st, zk_r1cs_verdict* out);
zk_status zk_r1cs_stage(const zk_r1cs* circuit, uint32_t constraint, uint32_t* stage_out, uint32_t* first_out,
                        uint32_t* count_out, char* name_out, size_t name_cap);

/* gen_proof of the anonymous transfer (ProofBuilder::gen_proof, core/proofs/src/anonymous.rs:97-183): the key
 * derivations of the confidential entry, the anonymity set assembled with the sender at s_index, the recipient at
 * t_index and the ten decoys in their order elsewhere (:117-126), MultiCiphertexts::<Anonymous>::encrypt
 * (crypto_components.rs:168-220: -amount under the sender's key, +amount under the recipient's, zero under every
 * decoy's, one randomness), the proof, check_proof over the 104 public coordinates (:213-264; ZK_ERR_UNSATISFIABLE if
 * it fails) and the packing of AnonymousXt (gen_xt :278-348, the struct :351-359).  enc_balances_* are indexed by set member.
 * zk_anonymous_derive is the host half alone (request -> statement and rsk). */
typedef struct {
    uint32_t amount, remaining_balance, s_index, t_index;
    uint8_t spending_key[32];
    uint8_t enc_key_recipient[32], enc_keys_decoy[ZK_ANONYMOUS_SIZE - 2][32];
    uint8_t enc_balances_left[ZK_ANONYMOUS_SIZE][32], enc_balances_right[ZK_ANONYMOUS_SIZE][32];
    uint8_t g_epoch[32];
    uint8_t randomness[32], alpha[32];
} zk_anonymous_request;
typedef struct {   /* AnonymousXt, anonymous.rs:351-359 */
    uint8_t proof[192];
    uint8_t enc_keys[ZK_ANONYMOUS_SIZE][32], left_ciphertexts[ZK_ANONYMOUS_SIZE][32];
    uint8_t right_ciphertext[32], nonce[32], rsk[32], rvk[32];
} zk_anonymous_xt;
zk_status zk_anonymous_derive(const zk_anonymous_request* req, size_t n, zk_anonymous_statement* statements_out, uint8_t* rsk_out);
/* zk_anonymous_derive_dev: zk_anonymous_derive as a stage on `device` (csrc/anon_derive.h), the front end of
 *   zk_anonymous_gen_proof_batch reachable on its own.  statements_out (n) and rsk_out (n x 32) are byte for byte what
 *   zk_anonymous_derive writes.  inputs_out (may be NULL) is n x 104 x 32 bytes: the public inputs of check_proof
 *   (anonymous.rs:213-264) as plain little-endian Fr, x then y of the twelve enc_keys, the twelve left ciphertexts, the balances'
 *   left halves, their right halves, the right ciphertext, rvk, g_epoch and the nonce - the order zk_verify_batch takes them for
 *   this circuit.  Neither the reference nor zk_anonymous_derive hands them out: with them zk_verify_batch checks a proof of a
 *   derived statement without deriving again.
 *   Up to ZKAMD_ANON_DERIVE_HOST_MAX requests (read per call; 0 = always the kernels) the whole derivation runs on the
 *   zk_set_host_threads pool, as zk_anonymous_derive's.  Above it the host keeps what reads the spending key - the checks of the
 *   indices and the three scalars, pgk = [sk] G, dec_key, rsk, and u = randomness dec_key - amount in Fs - and the device does the
 *   rest in two launches: every DISTINCT encoding of the batch decoded and tested for prime order once, [randomness] key for the
 *   recipient and the decoys and [dec_key] g_epoch with a scalar per lane, five multiplications by G per request over a resident
 *   table, then one lane per output point.  The spending key never reaches the device: what travels is what the statement carries
 *   to the witness kernels anyway (randomness, alpha, dec_key), with u and the amount.  Those buffers live for the call and are
 *   zeroed before it returns (zk_memory_stats counts them), on failure too; host copies are wiped.  The host form multiplies
 *   without branching on a scalar; the device form is NOT constant-time: a zero digit of a lane's scalar skips that lane's addition.
 *   Both forms write the same bytes and refuse the same requests: ZK_ERR_INVALID_ARGUMENT with zk_anonymous_derive's message for
 *   the lowest failing request - its indices, then its three scalars, then the first of its points, in the order recipient,
 *   decoys, g_epoch, enc_balances_left[i], enc_balances_right[i], that does not decode or lies outside the prime-order subgroup.
 *   After a refusal the outputs hold nothing to rely on.  n == 0 is ZK_OK and touches nothing; a NULL req, statements_out or
 *   rsk_out with n > 0 is "null argument"; a device out of range is ZK_ERR_INVALID_ARGUMENT in either form. */
zk_status zk_anonymous_derive_dev(const zk_anonymous_request* req, size_t n, int device, zk_anonymous_statement* statements_out,
                                  uint8_t* rsk_out, uint8_t* inputs_out);
/* the two scans (declared with zk_elgamal_decrypt above, where their results are) */
zk_status zk_confidential_scan(zk_elgamal_table* t, size_t n, const zk_confidential_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                               zk_confidential_scan_result* out);
zk_status zk_anonymous_scan(zk_elgamal_table* t, size_t n, const zk_anonymous_xt* xts, const uint8_t dec_key[32], uint64_t limit,
                            zk_anonymous_scan_result* out);
/* The two scans for a SET of decryption keys - an exchange's, a custodian's, an auditor's - in one call.  The reference has no
 * counterpart; the parts are those of the two scans (keys.rs:250-261, elgamal.rs:85-108, crypto_components.rs:168-220).
 * zk_scan_keys_create: dec_keys is n_keys x 32 bytes, little-endian, n_keys >= 1.  Every key must be a canonical Fs scalar (else
 *   ZK_ERR_INVALID_ARGUMENT naming its index) and no two may be equal (else ZK_ERR_INVALID_ARGUMENT naming both indices: a key set
 *   is a set).  The handle holds the scalars, the 32 canonical bytes of EncryptionKey::from_decryption_key for each - derived
 *   once, here, on the zk_set_host_threads pool, not per block - and an index from those bytes to the key's number.  Like the
 *   single-key entries it takes decryption keys alone, so a caller cannot hand over a pair that does not belong together.  It is
 *   host-only and binds no device.  zk_scan_keys_free wipes the scalars before releasing them (NULL: nothing).
 * zk_scan_keys_get: the derived encryption keys of keys first .. first + count - 1 (count x 32 bytes); a range outside the set is
 *   ZK_ERR_INVALID_ARGUMENT.
 * zk_confidential_scan_keys / zk_anonymous_scan_keys: a hit is a pair (extrinsic i, key k) in which key k's 32 bytes equal
 *   enc_key_sender or enc_key_recipient of xts[i] (one of the twelve enc_keys for the anonymous scan).  hits_out[h] names the
 *   pair (xt, key) and r is, byte for byte, what zk_confidential_scan / zk_anonymous_scan writes into out[i] for dec_key k: role
 *   or members, the found bits, the values or delta, and the refusal byte with its push order.  An extrinsic can be hit by
 *   several keys: a transfer between two keys of the set gives two hits, a transfer to oneself ONE hit with role 3, a ring up to
 *   twelve.  Hits are ordered by xt ascending, then key ascending.  Pairs that do not match produce nothing, and nothing of an
 *   extrinsic without a hit is looked at.
 *   Matching happens on the host first: with more hits than hits_cap the call fails with ZK_ERR_INVALID_ARGUMENT, *n_hits_out
 *   holds the number needed, hits_out is untouched and no other work is started.  2 n (confidential) / 12 n (anonymous) always
 *   suffices.  On success *n_hits_out is the number of hits written; on any other failure it is 0.
 *   limit and ZKAMD_SCAN_HOST_MAX are those of the single-key entries: up to that many values to decrypt the point work - once
 *   per HIT: dec_key k * right - runs on the host threads, above it in two kernels on the table's device (csrc/scan_keys.h), whose
 *   lanes each carry the scalar of their own hit; the bytes written do not depend on the form.  The scalars of the hits, and
 *   everything derived from them, travel per call: they are wiped on the host and zeroed on the device before the call returns,
 *   and nothing of the key set stays on the device between calls.  The host form multiplies without branching on a key; the
 *   device form is NOT constant-time: a zero digit of a lane's scalar skips that lane's addition.
 *   t == NULL, keys == NULL, n_hits_out == NULL, a NULL xts with n > 0, or a NULL hits_out with hits to write:
 *   ZK_ERR_INVALID_ARGUMENT ("null argument").  n == 0 sets *n_hits_out = 0 and touches nothing else. */
typedef struct zk_scan_keys zk_scan_keys;
zk_status zk_scan_keys_create(const uint8_t* dec_keys, size_t n_keys, zk_scan_keys** out);
zk_status zk_scan_keys_get(const zk_scan_keys* k, size_t first, size_t count, uint8_t* enc_keys_out);  /* count x 32 bytes */
void zk_scan_keys_free(zk_scan_keys* k);
typedef struct { uint32_t xt, key; zk_confidential_scan_result r; } zk_confidential_scan_hit;  /* 24 bytes */
typedef struct { uint32_t xt, key; zk_anonymous_scan_result r; } zk_anonymous_scan_hit;        /* 24 bytes */
zk_status zk_confidential_scan_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n, const zk_confidential_xt* xts,
                                    uint64_t limit, zk_confidential_scan_hit* hits_out, size_t hits_cap, size_t* n_hits_out);
zk_status zk_anonymous_scan_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n, const zk_anonymous_xt* xts,
                                 uint64_t limit, zk_anonymous_scan_hit* hits_out, size_t hits_cap, size_t* n_hits_out);
zk_status zk_anonymous_gen_proof_batch(zk_params* p, zk_r1cs* circuit, struct zk_vk* vk, size_t n, const zk_anonymous_request* req,
                                       const uint8_t* rs, zk_anonymous_xt* out);

/* ------------------------------------------------------------------------------------------
 * Parameter generation  (bellman groth16::generate_parameters(circuit, g1, g2, alpha, beta, gamma, delta, tau))
 * replaces: generate_random_parameters   reference calls: core/proofs/src/setup.rs:28-31, 59-62
 * The circuit is the R1CS held by `circuit` (zk_r1cs_load / zk_transfer_r1cs_load); the per-input rows
 * Input(i) * 0 = 0 are appended as bellman's generator appends them.  g1 / g2: the generators (uncompressed; bellman
 * draws them at random, any generators do), the five trapdoor scalars: 32 bytes little-endian plain < r.
 * out receives Parameters::write bytes (zk_params_load reads them back); out may be NULL to query the length.
 * Lagrange coefficients by the prover's NTT, QAP evaluation and all fixed-base multiplications on the GPU.
 * ZK_ERR_UNCONSTRAINED_VARIABLE as bellman (an aux variable whose L query is the identity),
 * ZK_ERR_UNEXPECTED_IDENTITY for gamma = 0 or delta = 0.
 * ------------------------------------------------------------------------------------------ */
zk_status zk_generate_parameters(zk_r1cs* circuit, const uint8_t g1[96], const uint8_t g2[192], const uint8_t alpha[32],
                                 const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta[32],
                                 const uint8_t tau[32], uint8_t* out, size_t cap, size_t* len);

/* ------------------------------------------------------------------------------------------
 * Verification  (bellman-verifier: prepare_verifying_key / verify_proof, PreparedVerifyingKey IO)
 * replaces: prepare_verifying_key + verify_proof   core/bellman-verifier/src/verifier.rs:15-63
 *           (called by the wallet's self-check core/proofs/src/confidential.rs:208-278 and by the
 *           runtime, modules/zk-system/src/lib.rs:57-108)
 * A zk_vk is a PreparedVerifyingKey resident on the GPU: e(alpha, beta), the line coefficients of
 * -gamma and -delta, the doubling tables of ic.
 *   zk_params_write_vk  VerifyingKey::write of the key inside a loaded Parameters (the first bytes of the
 *                       parameter file: alpha_g1 | beta_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2 | n_ic | ic)
 *   zk_vk_prepare       VerifyingKey bytes -> prepare_verifying_key (pairing and G2 preparation on the GPU)
 *   zk_vk_read / write  PreparedVerifyingKey::read / write (core/bellman-verifier/src/lib.rs:175-244; the
 *                       reference's zface/params/conf_vk.dat is such a file)
 *   zk_verify_batch     n independent verify_proof calls (eighteen lanes per Fq12 element, csrc/pairing.h): proofs n x 192 bytes
 *                       (Proof::read: compressed points, curve and subgroup checks), public inputs
 *                       n x n_inputs x 32 bytes (plain little-endian, WITHOUT the leading ONE).
 *                       ok_out[i] = 1 iff proof i verifies; a malformed proof or input is 0, not an error.
 *                       ZK_ERR_MALFORMED_VERIFYING_KEY if n_inputs + 1 != ic length (verifier.rs:38-40).
 *                       The entry picks the faster of the two forms per chunk itself (round 6): the per-proof check below 4096
 *                       proofs, the combined check of zk_verify_batch_rlc from there on (measured crossover, verify.cpp
 *                       VERIFY_RLC_AUTO_MIN) - the verdicts are the same either way.
 * ------------------------------------------------------------------------------------------ */
typedef struct zk_vk zk_vk;
zk_status zk_params_write_vk(const zk_params* p, uint8_t* out, size_t cap, size_t* len);
zk_status zk_vk_prepare(const uint8_t* vk_bytes, size_t len, int device, zk_vk** out);
zk_status zk_vk_read(const uint8_t* pvk_bytes, size_t len, int device, zk_vk** out);
/* out may be NULL to query the length */
zk_status zk_vk_write(const zk_vk* vk, uint8_t* out, size_t cap, size_t* len);
zk_status zk_vk_num_inputs(const zk_vk* vk, uint32_t* n_inputs);
void zk_vk_free(zk_vk* vk);
zk_status zk_verify_batch(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs,
                          uint8_t* ok_out);
/* The same verdicts through a random linear combination of the batch (bellman's batch verifier):
 *     prod_i e(rho_i A_i, B_i) * e(sum_i rho_i acc_i, -gamma) * e(sum_i rho_i C_i, -delta) == e(alpha, beta)^(sum_i rho_i)
 * - n + 2 Miller loops and ONE final exponentiation per chunk of up to 8192 proofs instead of 3 n and n.  rho_i = 128 bits of
 * Blake2s over the batch itself (proofs, inputs, index): no randomness source, a wrong accept has probability 2^-128 per
 * attempt.  A chunk that holds a malformed or invalid proof - or whose combined check fails - is handed to the per-proof
 * verifier, which names the culprits: ok_out is ALWAYS what zk_verify_batch would have written.  Pays on large batches
 * (throughput); for a few hundred proofs the per-proof entry is as fast (both are one chain of serial stages). */
zk_status zk_verify_batch_rlc(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs,
                              uint8_t* ok_out);
zk_status zk_verify_proof(zk_vk* vk, const uint8_t proof[192], const uint8_t* public_inputs, size_t n_inputs, int* ok);
/* Proof::read (core/bellman-verifier/src/lib.rs:67-110) for n proofs of 192 bytes, without the pairing: is every
 * point a well-formed compressed encoding (ec.rs:785-837, :1438-1518) of a curve point in the r-torsion subgroup that
 * is not the point at infinity?  status_out[i] = 0 when Proof::read would succeed, else
 * (which point: 1 = A, 2 = B, 3 = C) | (reason << 2) for the first point that fails.  vk supplies the device and
 * the workspaces; its key material is not used. */
enum { ZK_PROOF_BAD_ENCODING = 1, ZK_PROOF_NOT_ON_CURVE = 2, ZK_PROOF_NOT_IN_SUBGROUP = 3, ZK_PROOF_INFINITY = 4 };
zk_status zk_proof_read_batch(zk_vk* vk, size_t n, const uint8_t* proofs, uint8_t* status_out);

/* ------------------------------------------------------------------------------------------
 * Verification of transfer extrinsics from their bytes (the runtime's side: modules/zk-system/src/lib.rs:56-165).
 * The public inputs of a transfer proof are the affine coordinates of the Jubjub points the extrinsic carries;
 * PublicInputBuilder::push (modules/zk-system/src/input_builder.rs:15-27) forms them with IntoXY, which is where a
 * verifier that starts from bytes spends its time (a square root in Fr and a 252-bit scalar multiplication per point).
 * ------------------------------------------------------------------------------------------ */
/* IntoXY (core/primitives/src/{enc_key,nonce,..}.rs into_xy; edwards.rs:92-165 read, :319-330 as_prime_order) for n encodings.
 * points: n x 32 bytes.  xy_out: n x 64 bytes, x then y, each 32 bytes little-endian canonical (two consecutive public
 * inputs of zk_verify_batch); zeroed where refused.  status_out[i]: 0, or 1 = y not in the field (io::Error::NotInField),
 * 2 = no x for that y (NotOnCurve), 3 = not in the prime-order subgroup.  A refusal is a status, never an error.
 * device < 0, or n <= ZKAMD_INTO_XY_HOST_MAX (default 384): on the host threads (zk_set_host_threads); else one lane per point on
 * `device` (csrc/xt_inputs.h).  The bytes written do not depend on the form. */
enum { ZK_INTO_XY_NOT_IN_FIELD = 1, ZK_INTO_XY_NOT_ON_CURVE = 2, ZK_INTO_XY_NOT_PRIME_ORDER = 3 };
zk_status zk_jubjub_into_xy(const uint8_t* points, size_t n, int device, uint8_t* xy_out, uint8_t* status_out);
/* zk_system::verify_confidential_proof (modules/zk-system/src/lib.rs:56-115) for n extrinsics: the eleven points in the
 * reference's push order - 1 enc_key_sender, 2 enc_key_recipient, 3 left_amount_sender, 4 left_amount_recipient,
 * 5 right_randomness, 6 left_fee, 7 balance left, 8 balance right, 9 rvk, 10 g_epoch, 11 nonce - through IntoXY, then
 * verify_proof.  enc_balances: n x 64 bytes (the chain's stored Ciphertext of the sender; Ciphertext::zero() is two
 * identity encodings), NULL = each xt's own enc_balance field.  g_epochs: one 32-byte encoding (stride 0, decoded once)
 * or one per xt (stride 32).  ok_out[i] = 1 iff every input formed and the proof verifies.  refusal_out (may be NULL):
 * 0 when all inputs formed, else (field 1..11) | (status << 6) of the first point in push order that IntoXY refuses.
 * ZK_ERR_MALFORMED_VERIFYING_KEY unless the key has 22 inputs. */
zk_status zk_confidential_verify_batch(zk_vk* vk, size_t n, const zk_confidential_xt* xts, const uint8_t* enc_balances,
                                       const uint8_t* g_epochs, size_t g_epoch_stride, uint8_t* ok_out, uint8_t* refusal_out);
/* verify_anonymous_proof (:118-165): fields 1..12 enc_keys, 13..24 left_ciphertexts, 25..36 balances left, 37..48 balances
 * right, 49 right_ciphertext, 50 rvk, 51 g_epoch, 52 nonce; enc_balances: n x 12 x 64 bytes, required; 104 inputs. */
zk_status zk_anonymous_verify_batch(zk_vk* vk, size_t n, const zk_anonymous_xt* xts, const uint8_t* enc_balances,
                                    const uint8_t* g_epochs, size_t g_epoch_stride, uint8_t* ok_out, uint8_t* refusal_out);

/* ------------------------------------------------------------------------------------------
 * A block of confidential transfers executed in one call: encrypted_balances::confidential_transfer
 * (modules/encrypted-balances/src/lib.rs:25-96) for n extrinsics IN ORDER, over the stored state of the accounts they name, the
 * nonce pool and g_epoch.  The result - a verdict per extrinsic and the accounts to store - equals that of this loop over the
 * extrinsics; acc(k) is the account whose enc_key has the bytes k, the pool starts as nonce_pool:
 *   1. Signature.  sigs given and signature i (message i of msgs / msg_offsets as zk_redjubjub_verify_batch, key xts[i].rvk)
 *      does not verify: BAD_SIGNATURE, detail = the reason of zk_redjubjub_verify_batch.  Nothing else happens: the call is
 *      never dispatched (ensure_signed, lib.rs:36).  sigs == NULL: signatures are not this call's business.
 *   2. Stored account unreadable.  acc(sender) or acc(recipient) holds a balance or pending ciphertext that Ciphertext::read
 *      refuses (what zk_jubjub_into_xy decides): BAD_ACCOUNT, nothing else happens.  The outputs of an unreadable account that a
 *      dispatched extrinsic names are 64 zero bytes twice, as for the ledger's refused slot.  (So the balance - fields 7 and 8 of
 *      zk_confidential_verify_batch - is never the refused point of step 5.)
 *   3. Rollover (lib.rs:41-46, 133-170).  rollover(sender), then rollover(recipient): an account with ZK_BLOCK_ROLLOVER_DUE
 *      that has not rolled over in this block gets balance += pending, pending = Ciphertext::zero(), and ZK_BLOCK_ROLLED in its
 *      output flags.  This stays whatever happens to the extrinsic below.
 *   4. Nonce.  nonce is in the pool (equal bytes, as Vec<Nonce>::contains): NONCE_USED.  The reference assert!s here (lib.rs:49)
 *      and pushes an accepted nonce onto a COPY of the pool (lib.rs:69: nonce_pool() returns the vector by value); this entry does
 *      what those lines mean to do - a rejection, and a pool that grows with every accepted extrinsic of the block.
 *   5. Public inputs.  Those of verify_confidential_proof (the eleven fields of zk_confidential_verify_batch), balance_sender =
 *      acc(sender).balance as it stands at this moment.  A refused point: REFUSED_POINT, detail = field | status << 6.
 *   6. Proof.  verify_proof fails: INVALID_PROOF.
 *   7. ACCEPTED: the nonce joins the pool; acc(sender).balance -= (left_amount_sender, right_randomness) + (left_fee,
 *      right_randomness); acc(recipient).pending += (left_amount_recipient, right_randomness).
 * accounts_out[a] is account a after the loop, its ciphertexts as Point::write gives them (canonical); an account that no
 * dispatched extrinsic names is copied through, flags and all.  The caller stores the accounts, sets LastRollOver where ROLLED is
 * set, appends the nonces of the accepted extrinsics to its pool and pays the fees: storage, epochs and fees stay the runtime's.
 * A bad extrinsic is a verdict, never an error.  ZK_ERR_INVALID_ARGUMENT (the index in zk_last_error(), nothing written): an
 * extrinsic whose sender or recipient key is not among the accounts, two accounts with equal keys, a NULL buffer with a non-zero
 * count, offsets that decrease.  ZK_ERR_MALFORMED_VERIFYING_KEY unless the key has 22 inputs.  n == 0 copies the accounts through.
 * Exactness does not rest on the proof system's soundness: the call proceeds in rounds.  A round verifies, in one batch, every
 * extrinsic whose verdict is open, each against the balance it meets if every still-open predecessor is rejected; a sweep in
 * order settles those whose hypothesis held (the first open one always does).  A block in which no sender has two extrinsics
 * that pass steps 1-5 takes ONE round and verifies each proof at most once; an extrinsic settled at steps 1, 2, 4 or 5 is not
 * verified at all.  stats_out (may be NULL): rounds (0 when steps 1 and 2 settle everything), the proofs verified over all
 * rounds, and the distinct 32-byte encodings decoded - eight per extrinsic, four per account, g_epoch, each once.
 * Up to ZKAMD_INTO_XY_HOST_MAX distinct encodings (read per call) the point work runs on the host threads, above it on the key's
 * device (csrc/block_exec.h); the verification always runs on the key's device.  The bytes written do not depend on the form.
 * ------------------------------------------------------------------------------------------ */
#define ZK_BLOCK_ROLLOVER_DUE 1u   /* in:  last_rollover < current epoch (lib.rs:145) */
#define ZK_BLOCK_ROLLED       2u   /* out: rolled over by this block: the caller sets LastRollOver */
typedef struct {
    uint8_t enc_key[32];
    uint8_t balance[64], pending[64];  /* EncryptedBalance / PendingTransfer, left | right; None = Ciphertext::zero() */
    uint32_t flags;
} zk_block_account;
enum { ZK_BLOCK_ACCEPTED = 0, ZK_BLOCK_BAD_SIGNATURE = 1, ZK_BLOCK_NONCE_USED = 2, ZK_BLOCK_BAD_ACCOUNT = 3,
       ZK_BLOCK_REFUSED_POINT = 4, ZK_BLOCK_INVALID_PROOF = 5 };
typedef struct {
    uint8_t verdict;    /* ZK_BLOCK_* */
    uint8_t detail;     /* BAD_SIGNATURE: reason of zk_redjubjub_verify_batch; REFUSED_POINT: the refusal byte of
                           zk_confidential_verify_batch (field | status << 6); else 0 */
    uint16_t reserved;
} zk_block_verdict;
typedef struct { uint32_t rounds, proofs_verified, points_decoded, reserved; } zk_block_stats;
zk_status zk_confidential_block_execute(zk_vk* vk, size_t n, const zk_confidential_xt* xts,
    const uint8_t* sigs /* n x 64 or NULL: signatures are not this call's business */,
    const uint8_t* msgs, const uint64_t* msg_offsets /* as zk_redjubjub_verify_batch; vk of xt i = xts[i].rvk */,
    size_t n_accounts, const zk_block_account* accounts, size_t n_pool, const uint8_t* nonce_pool /* n_pool x 32 */,
    const uint8_t g_epoch[32], zk_block_account* accounts_out, zk_block_verdict* verdicts_out,
    zk_block_stats* stats_out /* may be NULL */);
/* ------------------------------------------------------------------------------------------
 * A block of anonymous transfers executed in one call: anonymous_balances::anonymous_transfer
 * (modules/anonymous-balances/src/lib.rs:23-82) for n extrinsics IN ORDER.  The arguments, zk_block_account, zk_block_verdict,
 * zk_block_stats, the ZK_BLOCK_* verdicts and the two flag bits are those of zk_confidential_block_execute.  The result equals
 * that of this loop over the extrinsics; acc(k) is the account whose enc_key has the bytes k, the pool starts as nonce_pool:
 *   1. Signature.  Exactly as step 1 above: sigs == NULL means signatures are not this call's business; a bad signature is
 *      BAD_SIGNATURE with the reason of zk_redjubjub_verify_batch, and nothing else happens.
 *   2. Stored account unreadable.  Any of the twelve acc(enc_keys[k]) holds a balance or pending ciphertext that Ciphertext::read
 *      refuses: BAD_ACCOUNT, nothing else happens - NO member of the ring is rolled over by this extrinsic.  (The convention of
 *      the confidential entry.  The reference's `for e in &enc_keys { rollover(e)? }` loop, lib.rs:37-39, would have rolled the
 *      members before the unreadable one.)  The outputs of an unreadable account that a dispatched extrinsic names are 64 zero
 *      bytes twice.
 *   3. Rollover (lib.rs:37-39, 169-206), for each of the twelve keys in order: an account with ZK_BLOCK_ROLLOVER_DUE that has not
 *      rolled over in this block gets balance += pending, pending = Ciphertext::zero(), and ZK_BLOCK_ROLLED.  A key that appears
 *      twice in a ring rolls once.  This stays whatever happens to the extrinsic below.
 *   4. Nonce.  nonce is in the pool: NONCE_USED (the reference assert!s, lib.rs:42; a rejection here, as above).  The pool grows
 *      with every accepted extrinsic.
 *   5. Public inputs.  The 52 fields of zk_anonymous_verify_batch; member k's balance is acc(enc_keys[k]).balance as it stands
 *      after step 3.  A refused point: REFUSED_POINT, detail = field | status << 6 of the first refused point in push order.
 *      Fields 25..48 are never the refused one: step 2 judged them.
 *   6. Proof.  verify_proof fails: INVALID_PROOF.
 *   7. ACCEPTED: the nonce joins the pool; for k = 0..11, acc(enc_keys[k]).pending += (left_ciphertexts[k], right_ciphertext).
 * accounts_out, the accounts no dispatched extrinsic names (copied through, flags and all), what stays the runtime's (storage,
 * epochs, LastRollOver) and the argument mistakes (ZK_ERR_INVALID_ARGUMENT with the index in zk_last_error(), nothing written: a
 * ring key that is not among the accounts, two accounts with equal keys, a NULL buffer with a non-zero count, offsets that
 * decrease) are as for the confidential entry.  ZK_ERR_MALFORMED_VERIFYING_KEY unless the key has 104 inputs.  n == 0 copies
 * the accounts through.
 * ONE verification batch is exact here.  Transfers only ever add to pending slots; a balance changes only by rollover, and
 * whether an account rolls over is known from signatures and stored bytes alone: rolled[a] = due[a] && (some extrinsic that
 * passes steps 1 and 2 names a).  An extrinsic that reaches step 5 has itself rolled every due member of its ring, so the balance
 * it meets for member a is rolled[a] ? balance + pending : balance - independent of its position and of every verdict.  The call
 * verifies, in one batch, every extrinsic that passes steps 1 and 2, whose nonce is not in the CALLER's pool and that has no
 * refused point; one sweep in order then applies steps 4 to 7 (a later twin of an accepted nonce is NONCE_USED although its
 * proof was checked).  stats_out (may be NULL): rounds = 1 if any extrinsic passes steps 1 and 2, else 0; proofs_verified = the
 * size of that batch; points_decoded = the distinct 32-byte encodings, each decoded once - 27 per extrinsic, four per account,
 * g_epoch.
 * Up to ZKAMD_INTO_XY_HOST_MAX distinct encodings (read per call) the point work runs on the host threads, above it on the key's
 * device (csrc/anon_block_exec.h); the verification always runs on the key's device.  The bytes written do not depend on the form.
 * ------------------------------------------------------------------------------------------ */
zk_status zk_anonymous_block_execute(zk_vk* vk, size_t n, const zk_anonymous_xt* xts,
    const uint8_t* sigs /* n x 64 or NULL */, const uint8_t* msgs, const uint64_t* msg_offsets,
    size_t n_accounts, const zk_block_account* accounts, size_t n_pool, const uint8_t* nonce_pool /* n_pool x 32 */,
    const uint8_t g_epoch[32], zk_block_account* accounts_out, zk_block_verdict* verdicts_out,
    zk_block_stats* stats_out /* may be NULL */);
/* ------------------------------------------------------------------------------------------
 * A block of encrypted-asset extrinsics executed in one call: the three dispatch functions of modules/encrypted-assets/src/lib.rs
 * - issue (:32-83), confidential_transfer (:86-164), destroy (:167-215) - for n extrinsics IN ORDER.  zk_confidential_xt,
 * zk_block_account, zk_block_verdict, zk_block_stats, the ZK_BLOCK_* verdicts, the two flag bits and the signature arguments
 * are those of zk_confidential_block_execute; the verifying key is the confidential one.  kinds[i] says which call extrinsic i
 * is, asset_ids[i] the id a transfer or destroy names.  An account of this module is keyed by (asset id, enc_key):
 * account_asset_ids[a] is the id of accounts[a], acc(c, k) the account with asset id c whose enc_key has the bytes k.  The
 * result equals that of this loop over the extrinsics; the pool starts as nonce_pool, the id counter as next_asset_id:
 *  TRANSFER (lib.rs:86-164): steps 1-7 of zk_confidential_block_execute with acc(asset_ids[i], .) in place of acc(.) - signature,
 *   an unreadable acc(id, sender) or acc(id, recipient) (BAD_ACCOUNT), rollover of both (:104-110, :266-304), nonce (:113),
 *   the public inputs against acc(id, sender).balance as it stands (:116-127), the proof, and sub_enc_balance /
 *   add_pending_transfer (:137-154, :307-358).
 *  ISSUE (lib.rs:32-83) reads enc_key_sender (the issuer), left_amount_sender (total), left_fee, enc_balance, right_randomness,
 *   rvk, nonce and proof; the recipient fields are not looked at.  It names no account and rolls nothing over.
 *   1. Signature, as step 1 of the confidential entry (ensure_signed, :42).
 *   2. Nonce in the pool (:49): NONCE_USED.
 *   3. Public inputs of verify_confidential_proof(issuer, issuer, total, total, enc_balance, rvk, fee, randomness, nonce) (:55-66)
 *      with the field numbers of zk_confidential_verify_batch: 1 = 2 = the issuer, 3 = 4 = total, 7 and 8 the halves of the
 *      extrinsic's OWN enc_balance - which CAN be the refused point here.  A refused point: REFUSED_POINT, detail =
 *      field | status << 6 of the first in push order.
 *   4. Proof: INVALID_PROOF.
 *   5. ACCEPTED (:72-82): the nonce joins the pool; the extrinsic gets the counter's value as its id and the counter goes up by
 *      one; effects_out[i].first = Ciphertext::from_left_right(total, randomness) as Point::write gives it - what
 *      EncryptedBalance((id, issuer)) and TotalSupply(id) get.  Storing them stays the caller's.
 *  DESTROY (lib.rs:167-215) reads the same fields, enc_key_sender as the owner, asset_ids[i] as the id.
 *   1. Signature (:178).
 *   2. acc(id, owner) unreadable: BAD_ACCOUNT.  (A convention, the one step 2 of the sibling entries chose: the reference
 *      would `take` without reading.)
 *   3. Nonce (:185): NONCE_USED.
 *   4. Public inputs (owner, owner, dummy_amount, dummy_amount, enc_balance, rvk, dummy_fee, randomness, nonce) (:189-200),
 *      dummy_amount = left_amount_sender, dummy_fee = left_fee; fields 7 and 8 as for an issue.
 *   5. Proof: INVALID_PROOF.
 *   6. ACCEPTED (:206-214): the nonce joins the pool; effects_out[i].first and .second are the account's balance and pending
 *      transfer as they stand (canonical); both then become Ciphertext::zero(), and ZK_BLOCK_TAKEN is set in the account's
 *      output flags.  A destroy does NOT roll its account over (:178-186), but it names it: the account's outputs are
 *      re-encoded canonically whatever the verdict past step 1.
 * What follows from the loop:
 *   - An account named first by a destroy and later by a transfer rolls over at the transfer, over the pending transfer as it
 *     stands then - zero after an accepted destroy, so the rollover moves nothing.  ZK_BLOCK_ROLLED is set whenever step 3 of a
 *     dispatched transfer reaches a due account.
 *   - None = Ciphertext::zero() throughout, exactly as in the confidential entry: after an accepted destroy a later subtraction
 *     subtracts from zero, where the reference's `and_then` (:321-328) would keep None.
 * accounts_out as for the confidential entry (an account no dispatched transfer or destroy names is copied through, flags and
 * all).  effects_out[i] of a rejected extrinsic: zeros, with the id it named (0 for an issue).  *next_asset_id_out: the counter
 * after the loop.  The caller stores accounts and issued balances, TotalSupply and NextAssetId, removes the entries of accounts
 * with ZK_BLOCK_TAKEN, deposits the events and pays the fees.
 * ZK_ERR_INVALID_ARGUMENT (the index in zk_last_error(), nothing written): a kind above 2; a transfer or destroy whose (id, key)
 * is not among the accounts; two accounts with equal (id, key); a NULL buffer with a non-zero count; offsets that decrease;
 * next_asset_id plus the number of issue extrinsics above UINT32_MAX; and ANY account, transfer or destroy whose asset id lies in
 * [next_asset_id, next_asset_id + the number of issue extrinsics of the call) - the ids this very call may assign, which keeps
 * the identity of every slot independent of the verdicts.  The caller's recourse: split the block in front of the named
 * extrinsic and hand each call the accounts its own extrinsics name; a call without an issue accepts every id, so splitting
 * ends.  ZK_ERR_MALFORMED_VERIFYING_KEY unless the key has 22 inputs.  n == 0 copies the accounts through and returns next_asset_id.
 * Rounds as in the confidential entry, the hypothesis of each being that every still-open predecessor is rejected.  Issues and
 * destroys take no balance from the ledger: only a still-open earlier extrinsic with the same nonce holds them, and each is
 * verified once.  A transfer waits for the next round when an earlier transfer from its account, or an earlier destroy of its
 * sender's account, is held or was accepted in this sweep, or an earlier extrinsic with its nonce is open.  ONE round for a
 * block in which no account sends twice and no destroy precedes a transfer from its account.  stats_out (may be NULL):
 * points_decoded = the distinct 32-byte encodings, each decoded once - eight per extrinsic, two more (enc_balance) for an issue
 * or destroy, four per account, g_epoch.
 * Up to ZKAMD_INTO_XY_HOST_MAX distinct encodings (read per call) the point work runs on the host, above it on the key's device,
 * where a scan that can forget (csrc/asset_block_exec.h) takes the place of the ledger's; the bytes do not depend on the form.
 * ------------------------------------------------------------------------------------------ */
#define ZK_BLOCK_TAKEN 4u      /* out: an accepted destroy took this account in this block */
enum { ZK_ASSET_TRANSFER = 0, ZK_ASSET_ISSUE = 1, ZK_ASSET_DESTROY = 2 };
typedef struct {               /* 136 bytes */
    uint32_t asset_id;         /* issue accepted: the id assigned; transfer, destroy: the id named; else 0 */
    uint32_t reserved;         /* 0 */
    uint8_t first[64];         /* issue accepted: Ciphertext::from_left_right(total, randomness), what EncryptedBalance
                                  and TotalSupply get; destroy accepted: the balance taken; else 64 zero bytes */
    uint8_t second[64];        /* destroy accepted: the pending transfer taken; else 64 zero bytes */
} zk_asset_effect;
zk_status zk_asset_block_execute(zk_vk* vk, size_t n, const zk_confidential_xt* xts,
    const uint8_t* kinds /* n: ZK_ASSET_* */, const uint32_t* asset_ids /* n: ignored for an issue */,
    const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
    size_t n_accounts, const zk_block_account* accounts, const uint32_t* account_asset_ids /* n_accounts */,
    size_t n_pool, const uint8_t* nonce_pool, const uint8_t g_epoch[32], uint32_t next_asset_id,
    zk_block_account* accounts_out, zk_block_verdict* verdicts_out, zk_asset_effect* effects_out,
    uint32_t* next_asset_id_out, zk_block_stats* stats_out /* may be NULL */);
/* The balance query at the head of a transfer (BalanceQuery::get_balance_from_decryption_key, zface/src/utils/getter.rs:135-175)
 * for the accounts of a key set in ONE call: EncryptedBalance + PendingTransfer (Ciphertext::add), the 64 bytes of the total
 * (Ciphertext::write), and Ciphertext::decrypt of it over [0, limit) with the search of zk_elgamal_decrypt on the table's device.
 * accounts: n_accounts x zk_block_account, what the block executors take and return - accounts_out of a block can be passed
 *   straight in; None is Ciphertext::zero(), the identity encoding twice.  A hit is an account whose enc_key has the 32 bytes of a
 *   key of `keys`; hits come in account order, and the same key may own several accounts (one per asset id): each is a hit.
 *   Nothing but the enc_key of an account without a hit is looked at.
 * The total of a hit is balance + pending where the account carries ZK_BLOCK_ROLLOVER_DUE - what the chain meets at the account's
 *   next extrinsic, and what the reference's getter always computes: set the bit everywhere for its behaviour - and balance alone
 *   where it does not; pending is then not read.  No other flag is looked at: accounts_out keeps the bit beside ZK_BLOCK_ROLLED on
 *   an account its block rolled over, and a caller that wants such an account read as the chain meets it next clears the bit where
 *   ROLLED is set, as it sets LastRollOver there.  enc_total is what a transfer request carries as enc_balance_left |
 *   enc_balance_right, value the number remaining_balance = value - amount - fee starts from.
 * A used point that Ciphertext::read refuses (what zk_jubjub_into_xy decides) is not an error of the call: the hit reports it in
 *   `refusal` and its neighbours are untouched.
 * hits_cap, n_hits_out and the NULL / n_accounts == 0 conventions are those of zk_confidential_scan_keys: matching runs first, on
 *   the host; with more hits than hits_cap the call fails with ZK_ERR_INVALID_ARGUMENT, *n_hits_out holds the number needed,
 *   hits_out is untouched and nothing is launched (hits_out = NULL, hits_cap = 0 is the sizing call; n_accounts always suffices).
 *   On success *n_hits_out is the number of hits written, on any other failure 0, and a half-written array never leaves the call.
 * limit 1 .. 2^32.  Up to ZKAMD_SCAN_HOST_MAX hits (the variable of the scans) the point work - decoding, the sums, one dec_key *
 *   right per hit - runs on the host threads, above it in two kernels on the table's device (csrc/balance_keys.h); the bytes
 *   written do not depend on the form.  The scalars of the hits and everything derived from them (dec_key * right, the point that
 *   is searched, the logarithms) travel per call: wiped on the host, zeroed on the device before the call returns, hits_out zeroed
 *   on failure.  The host form multiplies without branching on a key; the device form is NOT constant-time. */
typedef struct {
    uint8_t  found;          /* 1: value is the plaintext of enc_total; 0: no x < limit is (value = 0) */
    uint8_t  refusal;        /* 0, or field | status << 6 of the first refused point among those USED, in the order
                                1 balance left, 2 balance right, 3 pending left, 4 pending right (the zkxt::INTO_XY_* statuses,
                                the convention of the scans); then found = 0, value = 0, enc_total = 64 zero bytes */
    uint8_t  pending_added;  /* 1 where the account carried ZK_BLOCK_ROLLOVER_DUE */
    uint8_t  reserved;       /* 0 */
    uint32_t value;
    uint8_t  enc_total[64];  /* Ciphertext::write of the total, left | right */
} zk_balance_result;                                                    /* 72 bytes */
typedef struct { uint32_t account, key; zk_balance_result r; } zk_balance_hit;   /* 80 bytes */
zk_status zk_balance_keys(zk_elgamal_table* t, const zk_scan_keys* keys, size_t n_accounts, const zk_block_account* accounts,
                          uint64_t limit, zk_balance_hit* hits_out, size_t hits_cap, size_t* n_hits_out);

/* ------------------------------------------------------------------------------------------
 * Hierarchical key derivation (zface/src/derive/mod.rs, a ZIP32-style scheme): every account of a wallet is a child of one
 * extended key, and the watch-only half - an extended proof generation key - derives the same non-hardened children without any
 * spending key: what an exchange, a custodian or an auditor runs on the server that reads blocks.  All bytes are the reference's.
 * An extended key is ZK_HD_XKEY_BYTES = 73 bytes: depth (1) | parent_enckey_tag (4) | child_index (u32 LE) | chain_code (32) |
 *   key (32) - SpendingKey::write for an xsk (kind ZK_HD_XSK), ProofGenerationKey::write for an xpgk (ZK_HD_XPGK); mod.rs:125-134,
 *   219-228.  Another kind is ZK_ERR_INVALID_ARGUMENT.
 * zk_hd_master (mod.rs:48-64): I = BLAKE2b-512("Zerochain_Master", seed), the key SpendingKey::from_seed(I[0..32]), the chain code
 *   I[32..64], depth 0, tag 00000000, index 0.
 * zk_hd_xpgk_from_xsk (mod.rs:136-146): the same header with pgk = [sk] G, G = FixedGenerators::NoteCommitmentRandomness; the two
 *   arrays may be the same.
 * zk_hd_derive: the children indices[0 .. n) of ONE parent; an index of 2^31 or more is hardened (components.rs:57-74).
 *   I = prf_expand_vec(chain_code, [0x11], sk, i LE) for a hardened child, (chain_code, [0x12], pgk, i LE) otherwise; f =
 *   Fs::to_uniform(prf_expand(I[0..32], [0x13])); the child's chain code is I[32..64], its depth the parent's + 1, its tag the first
 *   four bytes of BLAKE2b-256("ZerochainEFinger", the parent's pgk); its key sk + f (xsk) or [f] G + pgk (xpgk).  The child's
 *   account (keys.rs:166-198): dec_key = BLAKE2s-256("zech_bdk", the child's pgk) with the top five bits of byte 31 cleared,
 *   enc_key = [dec_key] G.  Each output may be NULL (not wanted): xkeys_out n x 73 bytes, children of the parent's kind; dec_keys_out
 *   n x 32, little-endian; enc_keys_out n x 32, Point::write.  Repeated indices are allowed.  n == 0 is ZK_OK and touches nothing.
 *   ZK_ERR_INVALID_ARGUMENT, with nothing written: a hardened index with ZK_HD_XPGK (the reference returns Err for that child,
 *   mod.rs:166-169; the message names the first such position); a parent of depth 255 (depth + 1 overflows in the reference); an
 *   xsk whose key is not a canonical Fs scalar (SpendingKey::read, keys.rs:67-74); an xpgk whose point does not decode or is outside
 *   the prime-order subgroup (ProofGenerationKey::read, keys.rs:210-217); a NULL xkey or indices with n > 0.  No failure leaves a
 *   partly written output: the outputs are written last, after everything that can fail.
 *   The hashes run on the zk_set_host_threads pool.  The point work of n children - [f_i] G + pgk, [dec_key_i] G, two inversions and
 *   two encodings each - runs on those threads for device < 0 or n <= ZKAMD_HD_HOST_MAX (read per call; 0 = always the kernel),
 *   above that in one kernel on `device`, one lane per child (csrc/hd_keys.h); both forms write the same bytes.  Both kinds take the
 *   same device route: the device receives f_i and the parent's pgk, never a spending key.  f_i and dec_key_i are key-derived: the
 *   device buffers that held them are zeroed before the call returns (zk_memory_stats counts them), on failure too, and the host
 *   copies are wiped.  The host form multiplies without branching on a scalar; the device form is NOT constant-time: a zero digit
 *   of a lane's scalar skips that lane's addition.
 * zk_scan_keys_create_hd: the handle zk_scan_keys_create would build from the decryption keys of those children in index order,
 *   without deriving the encryption keys a second time; zk_scan_keys_get, both scans and zk_balance_keys work on it unchanged.  n
 *   must be 1 .. 2^32 - 1; two equal indices fail with zk_scan_keys_create's "dec_key a and dec_key b are equal".
 * zk_jubjub_base_mul_dev: n x [scalar_i] G, optionally + addend_i, ALWAYS in the kernel on `device` - the multiplier of the
 *   entries above, reachable with chosen scalars.  Scalars as zk_jubjub_base_mul: canonical Fs, else ZK_ERR_INVALID_ARGUMENT
 *   naming the index.  addends: n x 32 bytes or NULL; each is read as edwards::Point::read reads it, WITHOUT a subgroup test.  A
 *   refused addend is a status, never an error: status_out[i] is 0 or ZK_INTO_XY_NOT_IN_FIELD / ZK_INTO_XY_NOT_ON_CURVE, and the
 *   output point of a refused addend is 32 zero bytes.  status_out: n bytes, required with addends and not written without.  The
 *   buffers are treated as zk_hd_derive's; not constant-time.
 * ------------------------------------------------------------------------------------------ */
#define ZK_HD_XKEY_BYTES 73
#define ZK_HD_XSK 0u
#define ZK_HD_XPGK 1u
zk_status zk_hd_master(const uint8_t* seed, size_t len, uint8_t xsk_out[73]);
zk_status zk_hd_xpgk_from_xsk(const uint8_t xsk[73], uint8_t xpgk_out[73]);
zk_status zk_hd_derive(uint32_t kind, const uint8_t xkey[73], const uint32_t* indices, size_t n, int device, uint8_t* xkeys_out,
                       uint8_t* dec_keys_out, uint8_t* enc_keys_out);
zk_status zk_scan_keys_create_hd(uint32_t kind, const uint8_t xkey[73], const uint32_t* indices, size_t n, int device,
                                 zk_scan_keys** out);
zk_status zk_jubjub_base_mul_dev(const uint8_t* scalars, const uint8_t* addends, size_t n, int device, uint8_t* points_out,
                                 uint8_t* status_out);

/* GEpoch::group_hash (core/primitives/src/g_epoch.rs:102-110): the Jubjub group hash (core/jubjub/src/group_hash.rs:17-46,
 * find_group_hash curve/mod.rs:223-247) personalised "zcgepoch" over the four little-endian bytes of `epoch` and a counter byte
 * from 0 - the g_epoch every wallet and verifier entry takes.  Host only.  out: Point::write of the point. */
zk_status zk_g_epoch(uint32_t epoch, uint8_t out[32]);

/* ------------------------------------------------------------------------------------------
 * RedJubjub (core/jubjub/src/redjubjub.rs): the signature an extrinsic carries.  The wallet signs with the rsk the derive
 * and gen_proof entries return (confidential.rs:372-431); the runtime checks the signature against the account id, which
 * is the rvk, on every extrinsic (core/primitives/src/signature.rs:65-82).  G = FixedGenerators::Diversifier, the generator
 * of zk_jubjub_base_mul.  H*(a || b) = Fs::to_uniform(BLAKE2b-512 personalised "Zcash_RedJubjubH" over a then b).
 * Message i is msgs[msg_offsets[i] .. msg_offsets[i + 1]) (msg_offsets: n + 1 values; empty messages are allowed, msgs may
 * be NULL when all are; offsets that decrease are ZK_ERR_INVALID_ARGUMENT).
 * ------------------------------------------------------------------------------------------ */
/* PrivateKey::sign (redjubjub.rs:73-103) for n keys.  rsk: n x 32 bytes, canonical Fs (ZK_ERR_INVALID_ARGUMENT naming the
 * index otherwise; the reference panics).  t: n x 80 bytes, the T the reference draws from its RNG - the library never draws
 * randomness.  sigs_out: n x 64 bytes, Rbar | S with r = H*(T || M), Rbar = write(r G), S = r + H*(Rbar || M) rsk.
 * Host only, on the zk_set_host_threads pool.  No branch or table address depends on rsk, T or r (masked selection in the
 * fixed-base multiplication, masked reduction mod s); the final conditional subtraction inside the host Fr routines is
 * variable-time, as in the reference's own Fr.  rsk, r and what is derived from them are wiped before the call returns. */
zk_status zk_redjubjub_sign(size_t n, const uint8_t* rsk, const uint8_t* t, const uint8_t* msgs, const uint64_t* msg_offsets,
                            uint8_t* sigs_out);
/* PublicKey::read + PublicKey::verify (redjubjub.rs:118-155) for n signatures, one verdict each (not the reference's
 * all-or-nothing batch_verify).  vks: n x 32 bytes; sigs: n x 64 bytes.  ok_out[i] = 1 or 0; reason_out (may be NULL), in the
 * reference's order of tests: 0 accepted, 1 vk is not a point (Point::read fails: NotInField or NotOnCurve), 2 Rbar is not a
 * point, 3 Sbar >= s, 4 the equation [8]([c]vk + R - [S]G) == O fails, c = H*(Rbar || M) over Rbar's bytes as given.  A
 * refusal is a verdict, never an error.  As in the reference there is NO prime-order test: a key or an R with a torsion
 * component, the identity, and x = 0 encoded with the sign bit set are all accepted.
 * device < 0, or n <= ZKAMD_REDJUBJUB_HOST_MAX (default 320; read per call, 0 = always the kernels): on the host threads; else two kernels
 * on `device` (csrc/redjubjub.h) while the host hashes the messages.  The bytes written do not depend on the form. */
enum { ZK_REDJUBJUB_BAD_VK = 1, ZK_REDJUBJUB_BAD_R = 2, ZK_REDJUBJUB_BAD_S = 3, ZK_REDJUBJUB_BAD_EQUATION = 4 };
zk_status zk_redjubjub_verify_batch(size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* msgs,
                                    const uint64_t* msg_offsets, int device, uint8_t* ok_out, uint8_t* reason_out);

/* ------------------------------------------------------------------------------------------
 * Stand-alone kernels (micro-benchmark / test entries)
 * ------------------------------------------------------------------------------------------ */
/* multiexp over G1 / G2: sum_i scalars[i] * bases[i].   replaces bellman multiexp (FullDensity).
 * bases: n x 96 (G1) / n x 192 (G2) uncompressed; scalars: n x 32 plain LE; out: uncompressed. */
typedef struct zk_msm zk_msm;
zk_status zk_msm_create(int group /*1 = G1, 2 = G2*/, const uint8_t* bases, size_t n, int window_bits /*0 = auto*/,
                        int checked, int device, zk_msm** out);
/* The same handle WITHOUT the table of doublings (bases that are used once or a few times: only the n bases stay
 * resident): a scalar is recoded into odd signed digits of `window_bits` bits at fixed positions (0 = auto), one
 * bucket set per digit position, the position results folded with doublings - classic variable-base Pippenger. */
zk_status zk_msm_create_variable(int group, const uint8_t* bases, size_t n, int window_bits, int checked, int device,
                                 zk_msm** out);
zk_status zk_msm_run(zk_msm* m, const uint8_t* scalars, uint32_t flags, uint8_t* out);
/* scalars already in HBM (device pointer, n x 32 bytes); out is a host buffer */
zk_status zk_msm_run_dev(zk_msm* m, const void* d_scalars, uint32_t flags, uint8_t* out);
void zk_msm_free(zk_msm* m);
zk_status zk_msm_g1(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]);
zk_status zk_msm_g2(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[192]);
/* The one-shot entries keep a handle per (device, group) - decoded bases, sort and reduction workspaces, ~1.1 KB per base -
 * for the next call; a call over more than 2^21 bases releases it again by itself.  This releases all of them now. */
void zk_msm_cache_release(void);

/* EvaluationDomain transforms over Fr, n = 2^log_n.
 * zk_ntt_fr: in-place on a HOST buffer of plain LE scalars, natural order in and out, the four
 * bellman operations: inverse = 0, coset = 0 -> fft ; 1, 0 -> ifft ; 0, 1 -> coset_fft ;
 * 1, 1 -> icoset_fft. */
zk_status zk_ntt_fr(uint8_t* data, uint32_t log_n, int inverse, int coset);

typedef struct zk_ntt zk_ntt;
#define ZK_NTT_INVERSE 1u
#define ZK_NTT_COSET 2u
#define ZK_NTT_IN_BITREV 4u   /* input is in bit-reversed order (skips the permutation) */
#define ZK_NTT_OUT_BITREV 8u  /* leave the output in bit-reversed order */
zk_status zk_ntt_create(uint32_t log_n, int device, zk_ntt** out);
/* d_data: device pointer, batch x 2^log_n x 32 bytes, Montgomery-form Fr, transformed in place */
zk_status zk_ntt_run_dev(zk_ntt* t, void* d_data, uint32_t batch, uint32_t flags);
void zk_ntt_free(zk_ntt* t);

/* Raw Montgomery products on the device multiplier (field 0 = Fr: 32-byte limbs, 1 = Fq: 48-byte
 * limbs; little-endian limb arrays exactly as the reference stores Fr / Fq): out = a*b*R^-1.
 * Exists so the reference's literal field KATs can be run through the kernels' arithmetic. */
zk_status zk_debug_field_mul(int field, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (used by bench.py): HIP-event timing of named kernels on the library's
 * stream.  zk_profile_begin() arms it, zk_profile_get() synchronises and reports.
 * ------------------------------------------------------------------------------------------ */
void zk_profile_begin(void);
/* returns the number of launches of `kernel` recorded since begin; *total_ms their summed time */
int zk_profile_get(const char* kernel, double* total_ms);
void zk_profile_end(void);
/* Two of the generated assembly kernels (the G2 bucket accumulation, level 1 of the G1 bucket reduction) exist in two
 * forms: the first keeps a few values in scratch memory across the loop, the second is scratch-free (1-2 % slower on a
 * healthy device, 3x faster on a device whose runtime caps the waves of scratch-using dispatches).  zk_params_load times
 * both on the device when the first key is loaded there and keeps the choice for the process (ZKAMD_KERNEL_FORM = scratch |
 * free overrides).  forms_out[0 / 1] = the form in use for the G2 accumulation / the reduction (0 = first, 1 = scratch-
 * free); ms_out = the comparison [G2 first, G2 scratch-free, reduction first, reduction scratch-free], zeros before any key
 * was loaded on the device.  No reference counterpart. */
zk_status zk_kernel_forms(int device, uint32_t forms_out[2], float ms_out[4]);
/* What the library holds on the device and in page-locked host memory, and what it wiped: every buffer that can hold
 * key-derived data (assignments, scalar vectors, the witness kernels' scratch, the digits and bucket sums of a multiexp,
 * staging areas) is zeroed before it goes back to the runtime; only the tables of a key (CRS points, twiddles) are not.
 * out = [device bytes held, device bytes of such buffers released so far, device bytes zeroed before release,
 *        page-locked bytes held, page-locked bytes released, page-locked bytes zeroed before release].
 * out[1] == out[2] and out[4] == out[5] always.  No reference counterpart (the reference leaves its heap to the OS). */
void zk_memory_stats(uint64_t out[6]);
/* the HIP stream (hipStream_t) all work of this library is enqueued on */
void* zk_stream(void);
zk_status zk_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif /* ZKAMD_H */
