// The request -> statement derivation of the anonymous transfer (core/proofs/src/anonymous.rs:97-146; wallet.cpp
// anonymous_derive_one is the host form) as a stage with a device form: zk_anonymous_derive_dev, and the front end of
// zk_anonymous_gen_proof_batch.  Included by wallet.cpp below hd_keys.h and the host form, and by elgamal_encrypt.h.
//
// Per request the host form decodes 36 points (a square root and a multiplication by the group order each), multiplies 13 times
// by a scalar of its own and four times by G, and encodes 16 points.  The device form keeps on the host only what reads the
// spending key:
//   host    (zk_set_host_threads pool) the index and scalar checks in the host form's order, pgk = [sk]G, dk = BLAKE2s("zech_bdk",
//           pgk) & mask, rsk = sk + alpha, and u = r dk - amount in Fs.  THE SPENDING KEY NEVER REACHES THE DEVICE (the rule of
//           hd_keys.h): what travels is what the statement already carries to the witness kernels - randomness, alpha, dec_key -
//           with u, the amount and the public pgk.  Then the DISTINCT 32-byte encodings of the slice (zkstage::Encodings: the
//           recipient keys, decoys, g_epoch - normally one for the batch - and the 24 balance halves; the identity's encoding, the
//           balance of a fresh account, is one lane like any other).
//   device  derive_stage.h's two launches per slice of requests, the lanes of a request described as data:
//         decode       every DISTINCT encoding of the slice
//         variable     12 per request: [r] key for the recipient and the ten decoys, [dk] g_epoch for the nonce - r and dk read from
//                      the request's five pool scalars, which are uploaded once
//         fixed        5 per request, 43 windows each, one per pool scalar: [dk]G the sender's key, [u]G the sender's left
//                      ciphertext ([r][dk]G - [amount]G as ONE multiplication), [amount]G, [r]G the right ciphertext,
//                      [alpha]G + pgk = rvk (the addend as a table entry)
//         combine      16 per request, 24 words each: a source (+ an addend: [amount]G on the recipient's lane); no lane answers
//                      for a decode lane - the host reads their coordinates and statuses itself
//   host    the statuses walked in the host form's order - per request the recipient, decoys 0 .. 9, g_epoch, then
//           enc_balances_left[i], enc_balances_right[i] for i = 0 .. 11 - and the lowest failing request reported with the host
//           form's message; then the statement, rsk and the 104 public coordinates of check_proof (anonymous.rs:213-264).
// Both forms write the same bytes and refuse the same requests with the same status and message.
// Secrets: the scalars, the projective points and everything derived from them live in the DevBufs of the call's Stage, zeroed
// before they are released (zk_memory_stats counts them), on success and on every failure; host copies are wiped on every way out.  The
// device form is NOT constant-time: a zero digit of a lane's scalar skips that lane's addition; the host form multiplies with
// jubjub_var_mul / jubjub_fixed_mul, whose steps do not depend on the scalar.
#pragma once
#include "derive_stage.h"

namespace zkanon {

using zkrt::fail;
using zkstage::NONE;

// ZKAMD_ANON_DERIVE_HOST_MAX: requests up to which the host form runs (read per call; 0 = always the kernels).  Measured
// (profiles/r32_anon_derive_probe.json, 16 host threads, the 104 public inputs written): the device form is 3.23 ms at 1 request
// against 4.70 for the host form, 4.06 against 5.28 at 8, 4.72 against 39.2 at 64, 7.65 against 690 at 1024 and 20.9 against 2648
// at 4096 - at NO probed size is the host form the faster one, so the default is 0, always the kernels.
constexpr size_t HOST_MAX = 0;
constexpr size_t N_SET = ZK_ANONYMOUS_SIZE, N_PTS = 4 * N_SET + 4, N_PUB = 2 * N_PTS;
constexpr size_t ENC_PER_REQ = 3 * N_SET;       // recipient, ten decoys, g_epoch, 24 balance halves
constexpr uint32_t VAR_PER_REQ = 12, FIX_PER_REQ = 5, OUT_PER_REQ = 16;
constexpr uint32_t FIX_DK = 0, FIX_U = 1, FIX_AMOUNT = 2, FIX_R = 3, FIX_ALPHA = 4;   // the pool scalars of a request, and the fixed lane of each
constexpr uint32_t OUT_RIGHT = 12, OUT_RVK = 13, OUT_NONCE = 14, OUT_SENDER = 15, OUT_WORDS = 24;
constexpr size_t SLICE = 4096;   // requests per pair of launches
static_assert(N_PUB == 104 && ENC_PER_REQ == 36, "the public inputs of check_proof, the decodings of a request");

inline size_t host_max() {
    const char* e = getenv("ZKAMD_ANON_DERIVE_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
}

// ---- host side
// a b mod s for two SECRETS below s: every step adds, the addend taken under a mask
inline void fs_mul_ct(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    uint64_t acc[4] = {0, 0, 0, 0}, pick[4];
    WipeOnExit wipe_acc{acc, sizeof(acc)}, wipe_pick{pick, sizeof(pick)};
    for (int bit = 251; bit >= 0; bit--) {
        zkrj::fs_add_ct(acc, acc, acc);
        const uint64_t m = 0ull - ((a[bit >> 6] >> (bit & 63)) & 1ull);
        for (int i = 0; i < 4; i++) pick[i] = b[i] & m;
        zkrj::fs_add_ct(acc, pick, acc);
    }
    memcpy(out, acc, 32);
}
// a - v mod s for a < s and a 32-bit v
inline void fs_sub_small_ct(const uint64_t a[4], uint32_t v, uint64_t out[4]) {
    uint64_t neg[4];   // s - v, and 0 for v = 0
    WipeOnExit wipe_neg{neg, sizeof(neg)};
    zkhost::u128 bo = v;
    for (int i = 0; i < 4; i++) {
        const zkhost::u128 d = (zkhost::u128)FS_MOD[i] - bo;
        neg[i] = (uint64_t)d;
        bo = (d >> 64) & 1;
    }
    zkrj::fs_reduce_ct(neg);
    zkrj::fs_add_ct(a, neg, out);
}

// the fields of a request in the order the host form decodes them: k = 0 the recipient, 1 .. 10 the decoys, 11 g_epoch, then
// enc_balances_left[i], enc_balances_right[i] at 12 + 2 i, 13 + 2 i
inline const uint8_t* field_of(const zk_anonymous_request& rq, size_t k) {
    if (k == 0) return rq.enc_key_recipient;
    if (k <= 10) return rq.enc_keys_decoy[k - 1];
    if (k == 11) return rq.g_epoch;
    const size_t i = (k - 12) / 2;
    return (k - 12) % 2 ? rq.enc_balances_right[i] : rq.enc_balances_left[i];
}
inline std::string field_name(size_t k) {
    if (k == 0) return "enc_key_recipient";
    if (k <= 10) return "enc_keys_decoy[" + std::to_string(k - 1) + "]";
    if (k == 11) return "g_epoch";
    return std::string((k - 12) % 2 ? "enc_balances_right[" : "enc_balances_left[") + std::to_string((k - 12) / 2) + "]";
}
// the field that holds the key of set member m, m not the sender: the recipient's, or the decoys' in their order elsewhere
inline size_t key_field(const zk_anonymous_request& rq, size_t m) {
    if (m == rq.t_index) return 0;
    size_t j = m;
    if (rq.s_index < m) j--;
    if (rq.t_index < m) j--;
    return 1 + j;
}

// what the host keeps of a request between its first part and its last
struct Head {
    uint64_t dk[4], u[4], r[4], alpha[4];
    uint32_t pgk_entry[zkhd::ENTRY_WORDS];
};

// The device form for requests [0, n): st, rsk as zk_anonymous_derive writes them; inputs (or NULL): n x 104 x 32 bytes, plain;
// tail (or NULL): n x 96 bytes, Point::write of the right ciphertext, rvk and the nonce.
inline zk_status derive_device(const zk_anonymous_request* rq, size_t n, int device, zk_anonymous_statement* st, uint8_t* rsk, uint8_t* inputs,
                               uint8_t* tail) {
    ZK_TRY(zkrt::use_device(device));
    const uint32_t* tab = nullptr;
    ZK_TRY(zkhd::device_table(device, &tab));
    (void)zkwit::tables();
    // ---- the host part.  A request the checks refuse ends the batch there: what lies below it is still derived, since a point of
    // a lower request that is refused goes first.
    std::vector<Head> heads(n);
    WipeOnExit wipe_heads{heads.data(), n * sizeof(Head)};
    std::vector<std::string> refused(n);
    {
        zkrt::ProfScope ps("anon_derive_host");
        ZK_TRY(zkrt::for_each_status(n, 64, [&](size_t i) -> zk_status {
            const zk_anonymous_request& q = rq[i];
            const std::string who = "request " + std::to_string(i) + ": ";
            if (q.s_index >= N_SET || q.t_index >= N_SET || q.s_index == q.t_index) {
                refused[i] = who + "s_index and t_index must be two different members of the set";
                return ZK_OK;
            }
            uint64_t sk[4], prod[4], r[4];
            WipeOnExit wipe_sk{sk, sizeof(sk)}, wipe_prod{prod, sizeof(prod)}, wipe_r{r, sizeof(r)};
            Head& h = heads[i];
            zkrt::load_scalar_le(q.spending_key, sk);
            zkrt::load_scalar_le(q.alpha, h.alpha);
            zkrt::load_scalar_le(q.randomness, h.r);
            const char* bad = !fs_lt_mod(sk) ? "spending_key" : !fs_lt_mod(h.alpha) ? "alpha" : !fs_lt_mod(h.r) ? "randomness" : nullptr;
            if (bad) {
                refused[i] = who + bad + " is not a canonical Fs scalar";
                return ZK_OK;
            }
            zk_anonymous_statement& s = st[i];
            memset(&s, 0, sizeof(s));
            s.amount = q.amount;
            s.remaining_balance = q.remaining_balance;
            s.s_index = q.s_index;
            s.t_index = q.t_index;
            memcpy(s.randomness, q.randomness, 32);
            memcpy(s.alpha, q.alpha, 32);
            memcpy(s.g_epoch, q.g_epoch, 32);
            const zkwit::JPoint pgk = jubjub_fixed_mul(sk);
            jubjub_encode(pgk.x, pgk.y, s.proof_generation_key);
            zkhd::dec_key_of(s.proof_generation_key, h.dk);
            memcpy(s.dec_key, h.dk, 32);
            const zkhost::Fr e[3] = {pgk.y + pgk.x, pgk.y - pgk.x, pgk.x * pgk.y * zkwit::edwards_d().dbl()};
            memcpy(h.pgk_entry, e, 96);
            fs_mul_ct(h.r, h.dk, prod);
            fs_sub_small_ct(prod, q.amount, h.u);
            fs_add(sk, h.alpha, r);   // SpendingKey::into_rsk
            memcpy(rsk + 32 * i, r, 32);
            return ZK_OK;
        }));
    }
    size_t good = 0;
    while (good < n && refused[good].empty()) good++;

    // ---- slices of the requests below the first one refused
    size_t slice = SLICE;
    if (const char* e = zkrt::hook_env("ZKAMD_DEBUG_ANON_SLICE")) slice = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));   // test hook: several slices of a few requests
    zkstage::Stage S;   // the scalars and their multiples, on the device and in the upload's host copy: gone on every way out of this function
    std::vector<uint32_t> ids;
    for (size_t first = 0; first < good; first += slice) {
        const size_t np = std::min(slice, good - first);
        // the distinct encodings, and where each field of each request went
        zkstage::Encodings E(np * ENC_PER_REQ);
        ids.resize(np * ENC_PER_REQ);
        for (size_t i = 0; i < np; i++)
            for (size_t k = 0; k < ENC_PER_REQ; k++) ids[i * ENC_PER_REQ + k] = E.put(field_of(rq[first + i], k));
        const size_t nv = np * VAR_PER_REQ, nf = np * FIX_PER_REQ;
        S.begin({E.size(), nv, nf, nf, np, np * OUT_PER_REQ, OUT_WORDS, false, "anon_derive_upload", "anon_derive_points", "anon_derive_combine",
                 "anon_derive_download"});
        memcpy(S.enc, E.enc.data(), E.size() * 32);
        ZK_TRY(zkrt::for_each_status(np, 64, [&](size_t i) -> zk_status {
            const zk_anonymous_request& q = rq[first + i];
            const Head& h = heads[first + i];
            const uint32_t var0 = (uint32_t)(i * VAR_PER_REQ), pool0 = (uint32_t)(i * FIX_PER_REQ), fix0 = (uint32_t)nv + pool0;
            for (uint32_t k = 0; k < VAR_PER_REQ; k++) {   // the lane of field k: the recipient, the decoys, g_epoch
                memcpy(S.venc + (var0 + k) * 8, field_of(q, k), 32);
                S.vidx[var0 + k] = pool0 + (k == 11 ? FIX_DK : FIX_R);
            }
            uint32_t* sc = S.pool + pool0 * 8;
            memcpy(sc + 8 * FIX_DK, h.dk, 32);
            memcpy(sc + 8 * FIX_U, h.u, 32);
            sc[8 * FIX_AMOUNT] = q.amount;
            memcpy(sc + 8 * FIX_R, h.r, 32);
            memcpy(sc + 8 * FIX_ALPHA, h.alpha, 32);
            memcpy(S.addends + i * zkhd::ENTRY_WORDS, h.pgk_entry, 96);
            for (uint32_t j = 0; j < FIX_PER_REQ; j++) {   // [scalar j]G into slot fix0 + j, the request's pgk added to [alpha]G
                const uint32_t d[4] = {pool0 + j, (uint32_t)zkhd::WINDOWS, j == FIX_ALPHA ? (uint32_t)i : NONE, fix0 + j};
                memcpy(S.fix + (pool0 + j) * 4, d, 16);
            }
            auto source = [&](size_t lane, uint32_t from, uint32_t addend) {
                const uint32_t d[4] = {from, addend, 0, NONE};
                memcpy(S.src + (i * OUT_PER_REQ + lane) * 4, d, 16);
            };
            for (size_t m = 0; m < N_SET; m++)
                source(m, m == q.s_index ? fix0 + FIX_U : var0 + (uint32_t)key_field(q, m), m == q.t_index ? fix0 + FIX_AMOUNT : NONE);
            source(OUT_RIGHT, fix0 + FIX_R, NONE);
            source(OUT_RVK, fix0 + FIX_ALPHA, NONE);
            source(OUT_NONCE, var0 + 11, NONE);
            source(OUT_SENDER, fix0 + FIX_DK, NONE);
            return ZK_OK;
        }));
        ZK_TRY(S.run(tab));

        // ---- the statuses in the host form's order, then what the request's outputs are made of
        const uint32_t *xy = S.xy, *status = S.dstatus, *cout = S.out;
        ZK_TRY(zkrt::for_each_status(np, 64, [&](size_t i) -> zk_status {
            const size_t g = first + i;
            const zk_anonymous_request& q = rq[g];
            const uint32_t* id = &ids[i * ENC_PER_REQ];
            for (size_t k = 0; k < ENC_PER_REQ; k++)
                if (const uint32_t s = status[id[k]])
                    return fail(ZK_ERR_INVALID_ARGUMENT, "request " + std::to_string(g) + ": " + field_name(k) +
                                                             (s == zkxt::INTO_XY_NOT_PRIME_ORDER ? " is not in the prime-order subgroup" : " is not a Jubjub point"));
            zk_anonymous_statement& s = st[g];
            const uint32_t* co = cout + i * OUT_PER_REQ * OUT_WORDS;
            zkhost::Fr pub[N_PUB];   // x | y of the public points, Montgomery form, in the order of the circuit's inputs
            auto decoded = [&](size_t at, size_t k) { memcpy(&pub[2 * at], xy + (size_t)id[k] * 16, 64); };
            auto combined = [&](size_t at, uint32_t lane) { memcpy(&pub[2 * at], co + lane * OUT_WORDS + 8, 64); };
            for (size_t m = 0; m < N_SET; m++) {
                if (m == q.s_index) {
                    combined(m, OUT_SENDER);
                    memcpy(s.enc_keys[m], co + OUT_SENDER * OUT_WORDS, 32);
                } else {
                    decoded(m, key_field(q, m));
                    jubjub_encode(pub[2 * m], pub[2 * m + 1], s.enc_keys[m]);   // the canonical bytes, whatever came
                }
                combined(N_SET + m, (uint32_t)m);
                memcpy(s.left_ciphertexts[m], co + m * OUT_WORDS, 32);
                decoded(2 * N_SET + m, 12 + 2 * m);
                decoded(3 * N_SET + m, 13 + 2 * m);
                memcpy(s.enc_balances_left[m], q.enc_balances_left[m], 32);
                memcpy(s.enc_balances_right[m], q.enc_balances_right[m], 32);
            }
            combined(4 * N_SET, OUT_RIGHT);
            combined(4 * N_SET + 1, OUT_RVK);
            decoded(4 * N_SET + 2, 11);
            combined(4 * N_SET + 3, OUT_NONCE);
            for (size_t k = 0; inputs && k < N_PUB; k++) {
                const zkhost::Fr pl = pub[k].from_mont();
                memcpy(inputs + (g * N_PUB + k) * 32, pl.l, 32);
            }
            if (tail) {
                memcpy(tail + 96 * g, co + OUT_RIGHT * OUT_WORDS, 32);
                memcpy(tail + 96 * g + 32, co + OUT_RVK * OUT_WORDS, 32);
                memcpy(tail + 96 * g + 64, co + OUT_NONCE * OUT_WORDS, 32);
            }
            return ZK_OK;
        }));
    }
    if (good < n) return fail(ZK_ERR_INVALID_ARGUMENT, refused[good]);
    return ZK_OK;
}

// the host form, with the same outputs: anonymous_derive, then the coordinates and the tail from its AnonDerived
inline zk_status derive_host(const zk_anonymous_request* rq, size_t n, zk_anonymous_statement* st, uint8_t* rsk, uint8_t* inputs, uint8_t* tail) {
    if (!inputs && !tail) return anonymous_derive(rq, n, st, rsk, nullptr);
    std::vector<AnonDerived> der(n);
    ZK_TRY(anonymous_derive(rq, n, st, rsk, der.data()));
    return zkrt::for_each_status(n, 64, [&](size_t i) -> zk_status {
        for (size_t k = 0; inputs && k < N_PTS; k++) {
            const zkhost::Fr px = der[i].pub[k].x.from_mont(), py = der[i].pub[k].y.from_mont();
            memcpy(inputs + (i * N_PUB + 2 * k) * 32, px.l, 32);
            memcpy(inputs + (i * N_PUB + 2 * k + 1) * 32, py.l, 32);
        }
        if (tail) {
            const zkwit::JPoint* t = &der[i].pub[4 * N_SET];
            jubjub_encode(t[0].x, t[0].y, tail + 96 * i);
            jubjub_encode(t[1].x, t[1].y, tail + 96 * i + 32);
            jubjub_encode(t[3].x, t[3].y, tail + 96 * i + 64);
        }
        return ZK_OK;
    });
}
// the stage: the form by ZKAMD_ANON_DERIVE_HOST_MAX, on `device` (bound by the caller's use_device or here)
inline zk_status derive(const zk_anonymous_request* rq, size_t n, int device, zk_anonymous_statement* st, uint8_t* rsk, uint8_t* inputs, uint8_t* tail) {
    if (n == 0) return ZK_OK;
    ZK_TRY(zkrt::use_device(device));
    return n <= host_max() ? derive_host(rq, n, st, rsk, inputs, tail) : derive_device(rq, n, device, st, rsk, inputs, tail);
}

}  // namespace zkanon
