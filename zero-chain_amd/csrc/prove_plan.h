// The plan of one chunk of the prover (zkamd.cpp prove_chunk): which form of every stage runs and where every section of the
// merged C job and of the witness vector lies, as pure integer logic on (proofs in the chunk, the circuit's sizes, the groups
// of equal bases, the tunables) - nothing here touches the HIP runtime, so the CPU suite pins it (tests/test_prove_plan.py,
// through zk_hook_prove_plan).  Every form gives the same proof bytes, so a threshold that moves by accident passes every
// parity test and only changes what a call costs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace zkrt {

// Default of ZKAMD_FOLD_IN_MSM_MAX: the few-jobs limit of a launch set (msm_plan.h MSM_FEW_JOBS; zkamd.cpp, which sees both
// headers, holds the two equal - this header stays free of the multiexp's so that ntt.h can include it)
constexpr size_t PROVE_FOLD_IN_MSM_MAX = 128;

// The environment variables a chunk of the prover reads, each with its own parsing rule.  Read once per chunk and in this one
// place (the suites flip them between calls: nothing is static).
struct ProveTunables {
    size_t batch_chunk;          // ZKAMD_BATCH_CHUNK: proofs per launch set; ignored unless atoi() of it is > 0
    size_t host_chunk;           // ZKAMD_HOST_CHUNK: proofs per staged block of host assignments; 0 = not set (the same rule)
    size_t fold_in_msm_max;      // ZKAMD_FOLD_IN_MSM_MAX: largest chunk whose fold C = s A + C' rides in the C multiexp
    size_t g2_lone_max;          // ZKAMD_G2_LONE_MAX: largest chunk on the narrow G2 window of a proof made alone
    size_t host_normalize_max;   // ZKAMD_HOST_NORMALIZE_MAX: largest chunk whose into_affine runs on the host
    size_t split_min;            // ZKAMD_SPLIT_MIN: smallest chunk that runs its two G1 jobs as two launch sets
    bool no_overlap;             // ZKAMD_NO_OVERLAP (by presence): every launch on one stream
    bool trace_host;             // ZKAMD_TRACE_HOST (by presence): one stderr line per chunk

    static ProveTunables read() {
        auto env_chunk = [](const char* name, size_t dflt) {
            const char* e = getenv(name);
            return e && atoi(e) > 0 ? (size_t)atoi(e) : dflt;
        };
        auto env_n = [](const char* name, size_t dflt) {   // (measurement overrides: atoll when set, so an empty string is 0)
            const char* e = getenv(name);
            return e ? (size_t)atoll(e) : dflt;
        };
        ProveTunables t;
        // proofs per launch set: large chunks amortise the latency-bound tails (reduction trees, sorts);
        // the workspaces of a 1024-proof chunk of the Transfer circuit take ~35 GB of the 288 GB
        t.batch_chunk = env_chunk("ZKAMD_BATCH_CHUNK", 1024);
        t.host_chunk = env_chunk("ZKAMD_HOST_CHUNK", 0);
        t.fold_in_msm_max = env_n("ZKAMD_FOLD_IN_MSM_MAX", PROVE_FOLD_IN_MSM_MAX);
        t.g2_lone_max = env_n("ZKAMD_G2_LONE_MAX", 2);
        t.host_normalize_max = env_n("ZKAMD_HOST_NORMALIZE_MAX", 16);
        t.split_min = env_n("ZKAMD_SPLIT_MIN", 64);   // tests: 1 or 2
        t.no_overlap = getenv("ZKAMD_NO_OVERLAP") != nullptr;
        t.trace_host = getenv("ZKAMD_TRACE_HOST") != nullptr;
        return t;
    }
};

// Where every section of the two scalar vectors of a proof lies, in scalars.  One function computes it; ensure_maps (the
// index maps), prove_chunk (the strides of the jobs) and ntt.h k_build_scalars (the stores) all read it, so the three cannot
// disagree about which base gets which scalar.
//   witness vector (the A and B2 jobs):  [ inputs | aux | 1 | r | s | sums of the A groups (ga) | of the B2 groups (gb2) ]
//   C job:  [ H block (head) | aux | r z (nv) | r | (fold: s z (nv) | s | r s) | (derived: inputs) | r * sums of the B1 groups
//             (gb1) | (fold: s * sums of the A groups (ga)) ]
// head: bellman's m coefficients, or [s | e] of the live rows (2 n_rows) over the derived bases, whose input variables carry
// the c part of H (prover_binding.h ensure_derived).  fold: the job is C = s * A + C' itself, over the bases of the A query, alpha_1
// and delta_1 behind the r.  A section the form does not have is at offset 0 (k_build_scalars tests in_tail for that).
// Value pairs (prover_binding.h derived_pairs, value_pairs.h; all lengths 0 without them): two linked variables that hold the same
// value in a proof are one term over the sum of their two bases, whose slots lie behind everything above -
//   witness vector:  ... | the variables again, for the B2 job (nv) | pairs of the A query (pa) | of the B2 query (pb2) ]
//   C job:           ... | pairs of the L section (pl) | r * pairs of the B1 query (pb1) | (fold: s * pairs of the A query (pa)) ]
// (the A and B2 jobs read one vector and a pair may exist in one query only: with pairs the B2 job has its own copy of the
// variables' slots, so that each query zeroes what it merged and nothing else.)
struct CJobLayout {
    uint32_t n_in, n_aux, head, ga, gb2, gb1, fold, derived;   // what it was computed from
    uint32_t w_one, w_sum_a, w_sum_b2, wstride;                // witness vector: 1 (r, s behind it), the two blocks of sums
    uint32_t aux, rz, r;                                       // C job
    uint32_t sz, s, rs;                                        // ... with fold
    uint32_t in_tail;                                          // ... over the derived bases
    uint32_t sum_b1, sum_a;                                    // (the sums of the groups at the end: r * B1's, then s * A's with fold)
    uint32_t cstride;
    uint32_t pa, pb2, pl, pb1;                                 // value pairs per query (0: none)
    uint32_t w_end;                                            // witness vector: the end of the sums (its stride without pairs)
    uint32_t w_b2v, w_pair_a, w_pair_b2;                       // ... with pairs
    uint32_t pair_l, pair_b1, pair_a;                          // C job, with pairs (pair_a: with fold)
    // the bytes beside the pair slots (ntt.h k_build_scalars: the length of the term in the slot), per proof: the strides of
    // the array of the witness vector's slots [pa | pb2] and of the C job's [pl | pb1 | (fold: pa)]
    uint32_t sel_w, sel_c;
};

// The counts of value pairs per query, in the order the layout takes them
struct PairCounts {
    uint32_t a = 0, b2 = 0, l = 0, b1 = 0;
    bool any() const { return (a | b2 | l | b1) != 0; }
    // the same counts by query number, [a, b_g2, l, b_g1] (value_pairs.h Query): the one place that pairs names with numbers
    static PairCounts of(const uint32_t n[4]) {
        PairCounts pc;
        pc.a = n[0]; pc.b2 = n[1]; pc.l = n[2]; pc.b1 = n[3];
        return pc;
    }
    uint32_t operator[](int query) const { return query == 0 ? a : query == 1 ? b2 : query == 2 ? l : b1; }
};

inline CJobLayout cjob_layout(uint32_t n_in, uint32_t n_aux, uint32_t head, uint32_t ga, uint32_t gb2, uint32_t gb1, bool fold,
                              bool derived, const PairCounts& pc = PairCounts()) {
    const uint32_t nv = n_in + n_aux;
    CJobLayout L = {};
    L.n_in = n_in; L.n_aux = n_aux; L.head = head; L.ga = ga; L.gb2 = gb2; L.gb1 = gb1; L.fold = fold; L.derived = derived;
    L.w_one = nv;
    L.w_sum_a = nv + 3;
    L.w_sum_b2 = L.w_sum_a + ga;
    L.w_end = L.wstride = L.w_sum_b2 + gb2;
    L.pa = pc.a; L.pb2 = pc.b2; L.pl = pc.l; L.pb1 = pc.b1;
    if (pc.any()) {
        L.w_b2v = L.wstride;
        L.w_pair_a = L.w_b2v + nv;
        L.w_pair_b2 = L.w_pair_a + pc.a;
        L.wstride = L.w_pair_b2 + pc.b2;
    }
    uint32_t at = head;
    auto section = [&at](uint32_t len) { const uint32_t off = at; at += len; return off; };
    L.aux = section(n_aux);
    L.rz = section(nv);
    L.r = section(1);
    if (fold) {
        L.sz = section(nv);
        L.s = section(1);
        L.rs = section(1);
    }
    if (derived) L.in_tail = section(n_in);
    L.sum_b1 = section(gb1);
    if (fold) L.sum_a = section(ga);
    if (pc.any()) {
        L.pair_l = section(pc.l);
        L.pair_b1 = section(pc.b1);
        if (fold) L.pair_a = section(pc.a);
        L.sel_w = pc.a + pc.b2;
        L.sel_c = pc.l + pc.b1 + (fold ? pc.a : 0);
    }
    L.cstride = at;
    return L;
}

enum class PG1 { G1, G1_LONE, G1D, G1D_LONE };     // the G1 group of the C' jobs (zk_params): the key's or the derived set's
enum class PMap { MAP_C, MAP_CF, MAP_CD, MAP_CFD };   // its index map: key or derived (D) bases, without or with the fold (F)

struct ProvePlan {
    bool fold_in_msm;
    bool host_norm;
    bool g2_lone;
    bool split;
    bool one_stream;
    PG1 g1;
    PMap map;
    CJobLayout layout;
};

// np proofs of a circuit of n_in + n_aux variables and n_rows live rows under a key of domain m; ga, gb2, gb1: the groups of
// equal bases the maps in use were built with; derived: the four-transform form over the derived bases; pc: the value pairs
// that set carries (over the derived set only: the key's own tables are built before any circuit is known)
inline ProvePlan prove_plan(size_t np, uint32_t n_in, uint32_t n_aux, uint32_t n_rows, size_t m, uint32_t ga, uint32_t gb2,
                            uint32_t gb1, bool derived, const ProveTunables& tun, const PairCounts& pc = PairCounts()) {
    ProvePlan p;
    // A few proofs made alone carry the final fold C = s * A + C' INSIDE the C multiexp: s * A = s alpha_1 + sum (s z_i) A_i +
    // (r s) delta_1 is 15.6 k more terms over bases whose doublings are in the table (+19 % pairs in a launch whose duration is
    // the length of its longest task, not their number), where the fold's kernel (k_ct_scale_add) is a chain of 252 doublings and ~75 additions
    // of ONE point: 4.7 ms of a 7.4 ms proof under a 255-bit s (profiles/r06c_lone_baseline_random_rs_launch_list.txt).
    // A batch keeps the chain: one row per proof, hidden behind the other pipeline lane, no extra pairs.
    // Up to the few-jobs limit of a launch set (128 proofs): there the chain is exposed at the end of the call - 4.7 ms on
    // a call of 17.6 ms for 32 proofs - and 19 % more G1 pairs cost less.  ZKAMD_FOLD_IN_MSM_MAX overrides (measurements;
    // the emulation suite sends small batches through the chunk form of the fold).
    p.fold_in_msm = np <= tun.fold_in_msm_max;
    // into_affine of a handful of proofs: on the host (the encoder's to_affine), the kernels only export
    p.host_norm = np <= tun.host_normalize_max;
    p.g2_lone = np <= tun.g2_lone_max;
    // A batch runs the two G1 jobs of its proofs as two launch sets, each under the recoding width of its own size: the
    // C' jobs (65 k terms) on the main stream behind the H pipeline, the A jobs (15.6 k terms, witness scalars only)
    // on the side stream behind the G2 set.  A few proofs made alone keep
    // ONE set (fewer launches on their critical path): all C' jobs, then all A jobs - workgroup i of a launch runs on XCD
    // i mod 8 and the sort is one workgroup per job, so alternating A, C' would put every large job on the odd XCDs.
    p.split = np >= tun.split_min;
    p.one_stream = tun.no_overlap;
    p.g1 = derived ? (p.split ? PG1::G1D : PG1::G1D_LONE) : (p.split ? PG1::G1 : PG1::G1_LONE);
    p.map = derived ? (p.fold_in_msm ? PMap::MAP_CFD : PMap::MAP_CD) : (p.fold_in_msm ? PMap::MAP_CF : PMap::MAP_C);
    // the H block at the head of the C' job: bellman's m coefficients, or [s | e] of the live rows over the derived bases
    p.layout = cjob_layout(n_in, n_aux, derived ? 2 * n_rows : (uint32_t)m, ga, gb2, gb1, p.fold_in_msm, derived,
                           derived ? pc : PairCounts());
    return p;
}

}  // namespace zkrt
