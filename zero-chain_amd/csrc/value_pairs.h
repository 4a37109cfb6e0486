// Value pairs: which variables of a circuit tend to hold the same value as an earlier one (host, pure logic - no HIP).
//
// A conditional selection or a conditional addition of the transfer circuits copies a coordinate whenever its bit is 0, so
// about a quarter of the full-width values of a witness repeat what another variable of the same witness already holds.
// z_p P_p + z_j P_j = z_j (P_p + P_j) when z_p = z_j, and P_p + P_j depends on the key alone: the prover keeps one more base
// per LINKED pair of variables (prover_binding.h derived_pairs) and k_build_scalars (ntt.h) decides proof by proof, on the values,
// which links merge.  The links are static: the chains below are a function of the circuit alone.  They affect what a proof
// costs and never its bytes - the identity holds for every assignment.
// The same holds for a stretch of up to RUN_MAX consecutive members of a chain that hold one value, z (P_1 + ... + P_l): a base
// more per link and length (RUN_MAX below).
//
// The chains come from PROBES: the library's own host calculator (transfer_witness.h) on eight built-in statements with fixed
// seeds.  For every variable of a probe, the nearest earlier variable with the same full-width value is recorded; a link is
// kept when it is the same variable in every probe that has one.  Whether the two values ARE equal in a given proof follows
// a witness bit and is not decided here.
//
// A query only has terms for the variables that are dense in it, and a merged pair needs both: the variables of a run
// alternate between the A side and the B side of their gadget's constraints (the x of a running sum is dense in both, the
// product y2 x1 that repeats it in A only), so chains over ALL variables would pair across the queries and merge little in
// each.  There are three sets of chains, each over the variables of its query alone: A (inputs and A-dense aux), B (B-dense,
// for b_g1 and b_g2), L (aux).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <map>
#include <array>
#include <vector>
#include "transfer_witness.h"

namespace zkpairs {

using zkhost::Fr;

// the longest chain, in variables: the walk of k_build_scalars (ntt.h PAIR_WALK_MAX links) never reaches its cap
constexpr uint32_t CHAIN_MAX = 32;
constexpr int N_PROBES = 8;

// more than 64 bits in v and in r - v (Montgomery form in): what costs a full column of digits
inline bool full_width(const Fr& x) {
    const Fr v = x.from_mont(), w = (-x).from_mont();
    return (v.l[1] | v.l[2] | v.l[3]) != 0 && (w.l[1] | w.l[2] | w.l[3]) != 0;
}

// pred[i] = the link of variable i (an earlier variable) or -1: the nearest earlier variable among those of `in` (nv flags)
// with the same full-width value, where that is the same variable in every probe that has one
inline std::vector<int32_t> links_from_probes(const std::vector<std::vector<Fr>>& probes, const std::vector<uint8_t>& in) {
    const size_t nv = in.size();
    std::vector<int32_t> pred(nv, -1);
    std::vector<uint8_t> seen(nv, 0), clash(nv, 0);
    for (const std::vector<Fr>& z : probes) {
        if (z.size() != nv) continue;
        std::map<std::array<uint64_t, 4>, int32_t> last;
        for (size_t i = 0; i < nv; i++) {
            if (!in[i] || !full_width(z[i])) continue;
            const std::array<uint64_t, 4> key = {z[i].l[0], z[i].l[1], z[i].l[2], z[i].l[3]};
            auto it = last.find(key);
            if (it != last.end()) {
                if (seen[i] && pred[i] != it->second) clash[i] = 1;
                seen[i] = 1;
                pred[i] = it->second;
                it->second = (int32_t)i;
            } else {
                last.emplace(key, (int32_t)i);
            }
        }
    }
    for (size_t i = 0; i < nv; i++)
        if (clash[i]) pred[i] = -1;
    return pred;
}

// Links -> chains, in place: at most one successor per variable (the lowest variable that links to it keeps the link), chains
// of at most CHAIN_MAX variables (a longer one is cut: its next variable starts a chain of its own), every link to an earlier
// variable.  Returns succ.
inline std::vector<int32_t> chains_finalize(std::vector<int32_t>& pred) {
    const size_t nv = pred.size();
    std::vector<int32_t> succ(nv, -1);
    std::vector<uint32_t> depth(nv, 0);   // variables before this one in its chain
    for (size_t i = 0; i < nv; i++) {
        const int32_t p = pred[i];
        if (p < 0) continue;
        if ((size_t)p >= i || succ[p] >= 0 || depth[p] + 1 >= CHAIN_MAX) {
            pred[i] = -1;
            continue;
        }
        succ[p] = (int32_t)i;
        depth[i] = depth[p] + 1;
    }
    return succ;
}

// ---- the probes: statements whose every field is a fixed function of (seed, field) --------------------------------------
struct Seeded {
    uint64_t s;
    uint64_t next() {   // SplitMix64
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    void scalar(uint64_t (&v)[4]) {   // 250 bits: below the order of the Jubjub subgroup
        for (int i = 0; i < 4; i++) v[i] = next();
        v[3] &= (1ull << 58) - 1;
    }
    zkwit::JPoint point() {   // a multiple of the fixed generator: on the curve, in the subgroup
        uint64_t k[4];
        scalar(k);
        return zkwit::fixed_base_value(zkwit::fs_bits(k));
    }
};

inline std::vector<Fr> flat(const zkwit::Wit& w) {
    std::vector<Fr> z(w.inputs);
    z.insert(z.end(), w.aux.begin(), w.aux.end());
    return z;
}

inline std::vector<std::vector<Fr>> transfer_probes() {
    std::vector<std::vector<Fr>> out;
    for (int k = 0; k < N_PROBES; k++) {
        Seeded g{0x7a6b616d64000000ull + (uint64_t)k};
        zkwit::Statement s;
        s.amount = (uint32_t)g.next();
        s.remaining_balance = (uint32_t)g.next();
        s.fee = (uint32_t)g.next();
        g.scalar(s.randomness);
        g.scalar(s.alpha);
        g.scalar(s.dec_key);
        s.pgk = g.point();
        s.enc_key_recipient = g.point();
        s.enc_balance_left = g.point();
        s.enc_balance_right = g.point();
        s.g_epoch = g.point();
        zkwit::Wit w;
        zkwit::synthesize(s, w);
        out.push_back(flat(w));
    }
    return out;
}

inline std::vector<std::vector<Fr>> anonymous_probes() {
    std::vector<std::vector<Fr>> out;
    for (int k = 0; k < N_PROBES; k++) {
        Seeded g{0x7a6b616e6f6e0000ull + (uint64_t)k};
        zkwit::AnonStatement s;
        s.amount = (uint32_t)g.next();
        s.remaining_balance = (uint32_t)g.next();
        s.s_index = (uint32_t)(g.next() % zkwit::ANON_SIZE);
        s.t_index = (uint32_t)(g.next() % zkwit::ANON_SIZE);
        g.scalar(s.randomness);
        g.scalar(s.alpha);
        g.scalar(s.dec_key);
        s.pgk = g.point();
        s.g_epoch = g.point();
        for (size_t i = 0; i < zkwit::ANON_SIZE; i++) {
            s.enc_keys[i] = g.point();
            s.left_ciphertexts[i] = g.point();
            s.balance_left[i] = g.point();
            s.balance_right[i] = g.point();
        }
        zkwit::Wit w;
        zkwit::synthesize_anonymous(s, w);
        out.push_back(flat(w));
    }
    return out;
}

enum Circuit { TRANSFER = 0, ANONYMOUS = 1 };

// the probe witnesses of one of the two built-in circuits, built once per process
inline const std::vector<std::vector<Fr>>& circuit_probes(Circuit c) {
    if (c == TRANSFER) {
        static const std::vector<std::vector<Fr>> t = transfer_probes();
        return t;
    }
    static const std::vector<std::vector<Fr>> a = anonymous_probes();
    return a;
}
constexpr int N_CHAINS = 3;   // A, B, L

// The four queries that can have pair bases, in the order of the q arrays and of the bytes of the availability word that
// k_build_scalars reads, of count_merges below and of the test hooks.  b_g2 and b_g1 follow the chains of B.
enum Query { QA = 0, QB2 = 1, QL = 2, QB1 = 3 };
constexpr int N_QUERIES = 4;
constexpr int chain_of(Query q) { return q == QA ? 0 : q == QL ? 2 : 1; }   // its place among [A | B | L] in chains_of

// The chains of a circuit, [pred A | succ A | pred B | succ B | pred L | succ L] over its variables (inputs, then aux): a
// function of the probes and of which variables are dense in the A and in the B query
inline std::vector<int32_t> chains_of(const std::vector<std::vector<Fr>>& probes, uint32_t n_in, const std::vector<uint8_t>& a_dense,
                                      const std::vector<uint8_t>& b_dense) {
    const size_t nv = a_dense.size();
    std::vector<uint8_t> aux(nv, 0);
    for (size_t i = n_in; i < nv; i++) aux[i] = 1;
    std::vector<int32_t> out;
    for (const std::vector<uint8_t>* in : {&a_dense, &b_dense, (const std::vector<uint8_t>*)&aux}) {
        std::vector<int32_t> pred = links_from_probes(probes, *in);
        const std::vector<int32_t> succ = chains_finalize(pred);
        out.insert(out.end(), pred.begin(), pred.end());
        out.insert(out.end(), succ.begin(), succ.end());
    }
    return out;
}

// The longest stretch of a run that becomes ONE term z (P_1 + ... + P_l): a run is cut into blocks of RUN_MAX members (ntt.h
// k_build_scalars has the rule).  Every size follows from it: RUN_MAX - 2 more bases per link (prover_binding.h derived_pairs), as
// many alternates per pair slot (msm_types.h MsmSelRange::alt), one bit per length in the words of k_build_scalars.  2 ... 8; 2 is the
// rule of pairs alone.  (ZK_RUN_MAX: a second library for measurements.)
#ifndef ZK_RUN_MAX
#define ZK_RUN_MAX 4
#endif
constexpr uint32_t RUN_MAX = ZK_RUN_MAX;
static_assert(RUN_MAX >= 2 && RUN_MAX <= 8, "a term's length is a nibble and a bit of a byte in k_build_scalars");

// The word k_build_scalars reads per variable j beside q*[j]: a byte per query [a | b_g2 | l | b_g1], bit l - 1 set where the
// query has the base of the l chain members that end at j, l = 3 ... RUN_MAX (l = 2 is q*[j] >= 0)
inline uint32_t avail_byte(const int32_t* q, const int32_t* avail, uint32_t query, size_t j, uint32_t cap) {
    uint32_t b = q[j] >= 0 ? 2u : 0u;
    if (avail) b |= ((uint32_t)avail[j] >> (8 * query)) & 0xfcu & ((1u << cap) - 1u);
    return b;
}

// The rule of k_build_scalars (ntt.h) on one witness, counted: how many terms a query saves.  pred, succ: the chains of the
// query; q[j] >= 0 where it has the pair base of the link (pred[j], j); avail (or null: pairs alone): the words above, `query`
// the byte of this query in them; cap: the longest term, <= RUN_MAX.  The same blocks and the same split as the kernel's.
inline uint64_t count_merges(const int32_t* pred, const int32_t* succ, const int32_t* q, const int32_t* avail, uint32_t query,
                             const std::vector<Fr>& z, uint32_t cap = RUN_MAX) {
    uint64_t merged = 0;
    for (size_t j = 0; j < z.size(); j++) {
        if (z[j].is_zero()) continue;
        uint32_t t = 0;
        for (int32_t k = pred[j]; k >= 0 && t < CHAIN_MAX && z[k] == z[j]; k = pred[k]) t++;
        if (t % cap) continue;   // j starts a block
        uint32_t av[8], n = 1;
        av[0] = 0;
        for (int32_t k = succ[j]; n < cap && k >= 0 && z[k] == z[j]; k = succ[k]) av[n++] = avail_byte(q, avail, query, (size_t)k, cap);
        for (uint32_t s = 0; s < n;) {   // the longest term that starts at s and has its base, then on behind it
            uint32_t len = 1;
            for (uint32_t l = n - s; l >= 2; l--)
                if ((av[s + l - 1] >> (l - 1)) & 1u) {
                    len = l;
                    break;
                }
            merged += len - 1;
            s += len;
        }
    }
    return merged;
}

}  // namespace zkpairs
