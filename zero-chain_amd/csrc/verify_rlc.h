// libzkamd, the coefficients of the combined check of a chunk (verify.cpp verify_chunk_rlc; pairing.h, "Batch verification with
// a random linear combination"): the Fiat-Shamir derivation as integer logic on the host.  Nothing here touches HIP - the host
// threads come in as a count and a runner - so the suite pins every word of it without a GPU (tests/test_verify_rlc.py through
// zk_hook_rlc_coefs, tests/verify_rlc_main.cpp under the sanitizers).  A slip here passes every verdict test: a chunk the
// combined check does not vouch for goes to the per-proof verifier.  Part of verify.cpp's translation unit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "blake2s.h"
#include "host_math.h"

namespace zkrlc {

constexpr size_t LEAF = 256;   // proofs per leaf of the seed's hash

// lambda = -x^2 mod r, plain: a primitive cube root of unity of Fr, the eigenvalue of the endomorphism k_rlc_scale applies
inline zkhost::Fr lambda() {
    static const uint64_t RMOD[4] = ZK_FR_P_64;
    const unsigned __int128 x2 = (unsigned __int128)ZK_BLS_X_ABS * ZK_BLS_X_ABS;
    zkhost::Fr l = zkhost::Fr::zero();
    l.l[0] = (uint64_t)x2;
    l.l[1] = (uint64_t)(x2 >> 64);
    uint64_t bo = 0;
    for (int k = 0; k < 4; k++) {   // r - x^2
        const unsigned __int128 d = (unsigned __int128)RMOD[k] - l.l[k] - bo;
        l.l[k] = (uint64_t)d;
        bo = (uint64_t)(d >> 64) & 1u;
    }
    return l;
}

// What the device is handed for n proofs of n_inputs public inputs each.  It is the pageable source of asynchronous copies: it
// lives until the chunk's streams have been waited for.
struct Coefs {
    std::vector<uint32_t> rho;   // rho_i as a_i | b_i, 2 x 64 bits (rho_i = a_i + b_i lambda); a zero draw is replaced by 1
    std::vector<uint32_t> s;     // n_inputs + 1 scalars of 8 words, plain: s_0 = sum_i rho_i, s_j = sum_i rho_i x_ij
    uint32_t exp[8];             // the exponent of e(alpha, beta) in the same decomposed form: sum_i a_i | sum_i b_i (< n 2^64 each)
    uint32_t nbits;              // the bit length of the longer half, at least 1
};

// seed = Blake2s(key_digest | n | digests of the leaves), a leaf = LEAF consecutive proofs with their inputs behind its index;
// rho_i = 2 x 64 bits of Blake2s(seed | i).  The coefficients are fixed by the key, the proofs and the inputs they weigh, no
// randomness source is needed and a run can be repeated.  run(nth, work) calls work(t) for t = 0 .. nth - 1, on threads or not:
// the leaves are hashed side by side (7 MB in one stream was 7 ms of the 8192-proof call), and neither the seed nor the sums -
// addition in Fr is exact - depend on nth.  The inputs are canonical Fr (the caller has checked).
template <class Run>
inline Coefs coefs(const uint8_t key_digest[32], size_t n, uint32_t n_inputs, const uint8_t* proofs, const uint8_t* inputs, unsigned nth,
                   Run&& run) {
    static const uint8_t pers[8] = {'z', 'k', 'a', 'm', 'd', 'r', 'l', 'c'};
    const size_t ni = n_inputs;
    nth = std::max(nth, 1u);
    uint8_t seed[32];
    {
        const size_t n_leaves = (n + LEAF - 1) / LEAF;
        std::vector<uint8_t> dig(n_leaves * 32);
        auto leaf_work = [&](unsigned t) {
            for (size_t l = n_leaves * t / nth; l < n_leaves * (t + 1) / nth; l++) {
                const size_t lo = l * LEAF, cnt = std::min(LEAF, n - lo);
                zkhash::Blake2s h(pers);
                h.update_u64be(l);
                h.update(proofs + lo * 192, cnt * 192);
                h.update(inputs + lo * ni * 32, cnt * ni * 32);
                h.finish(&dig[l * 32]);
            }
        };
        run(nth, leaf_work);
        zkhash::Blake2s h(pers);
        h.update(key_digest, 32);
        h.update_u64be(n);
        h.update(dig.data(), dig.size());
        h.finish(seed);
    }
    Coefs c;
    c.rho.resize(n * 4);
    const zkhost::Fr lambda_m = lambda().to_mont();
    struct Part {
        std::vector<zkhost::Fr> s;
        unsigned __int128 sa = 0, sb = 0;
    };
    std::vector<Part> part(nth);
    for (auto& pt : part) pt.s.assign(ni + 1, zkhost::Fr::zero());
    auto work = [&](unsigned t) {
        for (size_t i = n * t / nth; i < n * (t + 1) / nth; i++) {
            uint8_t d[32];
            zkhash::Blake2s h;
            h.update(seed, 32);
            h.update_u64be(i);
            h.finish(d);
            uint32_t* rho = &c.rho[i * 4];
            memcpy(rho, d, 16);
            if (!(rho[0] | rho[1] | rho[2] | rho[3])) rho[0] = 1;
            uint64_t ab[2];
            memcpy(ab, rho, 16);
            part[t].sa += ab[0];
            part[t].sb += ab[1];
            zkhost::Fr a = zkhost::Fr::zero(), b = zkhost::Fr::zero();
            a.l[0] = ab[0];
            b.l[0] = ab[1];
            const zkhost::Fr rm = a.to_mont() + b.to_mont() * lambda_m;   // rho_i R
            part[t].s[0] = part[t].s[0] + rm;
            for (size_t j = 0; j < ni; j++) {
                zkhost::Fr x;
                memcpy(x.l, inputs + (i * ni + j) * 32, 32);   // plain: rho R * x / R = rho x, plain
                part[t].s[1 + j] = part[t].s[1 + j] + rm * x;
            }
        }
    };
    run(nth, work);
    c.s.resize((ni + 1) * 8);
    unsigned __int128 sa = 0, sb = 0;
    for (unsigned t = 0; t < nth; t++) {
        sa += part[t].sa;
        sb += part[t].sb;
    }
    for (size_t j = 0; j <= ni; j++) {
        zkhost::Fr a = zkhost::Fr::zero();
        for (unsigned t = 0; t < nth; t++) a = a + part[t].s[j];
        if (j == 0) a = a.from_mont();   // sum of rho_i R -> plain; the others are plain already
        memcpy(&c.s[j * 8], a.l, 32);
    }
    // e(alpha, beta)^(sum a_i) * (e(alpha, beta)^lambda)^(sum b_i)
    memcpy(&c.exp[0], &sa, 16);
    memcpy(&c.exp[4], &sb, 16);
    c.nbits = 128;
    while (c.nbits > 1 && !(((c.exp[(c.nbits - 1) >> 5] | c.exp[4 + ((c.nbits - 1) >> 5)]) >> ((c.nbits - 1) & 31)) & 1u)) c.nbits--;
    return c;
}

}  // namespace zkrlc
