// Binding a key to a circuit: the derived bases of a (key, circuit) pair with their value pairs and runs (ensure_derived,
// derived_pairs) and the index maps of a density pattern over them (ensure_maps).  Included by zkamd.cpp alone.
#pragma once
#include <atomic>
#include <chrono>
#include "prover_key.h"

namespace {

// Where the variables of a circuit lie in the A query and in the B queries (b_g1 and b_g2 alike), from the density trackers:
// bellman's generator emits exactly one `a` entry per input and per dense aux variable, and the b queries likewise.
struct QueryPositions {
    std::vector<int32_t> pos_a, pos_b;     // variable -> position in the query, -1 where it has no term
    std::vector<uint32_t> var_a, var_b;    // query position -> variable
    uint32_t n_a() const { return (uint32_t)var_a.size(); }
    uint32_t n_b() const { return (uint32_t)var_b.size(); }
};
QueryPositions query_positions(uint32_t n_in, uint32_t n_aux, const uint8_t* a_aux_d, const uint8_t* b_in_d, const uint8_t* b_aux_d) {
    const uint32_t nv = n_in + n_aux;
    QueryPositions Q;
    Q.pos_a.assign(nv, -1);
    Q.pos_b.assign(nv, -1);
    for (uint32_t i = 0; i < nv; i++) {
        if (i < n_in || a_aux_d[i - n_in]) {   // A inputs: full density
            Q.pos_a[i] = (int32_t)Q.var_a.size();
            Q.var_a.push_back(i);
        }
        if (i < n_in ? b_in_d[i] : b_aux_d[i - n_in]) {
            Q.pos_b[i] = (int32_t)Q.var_b.size();
            Q.var_b.push_back(i);
        }
    }
    return Q;
}
// Which variables occur in A (every input counts as one that does) and in B of a constraint system: what bellman's density
// trackers record of it
void system_densities(const zkr1cs::System& sys, std::vector<uint8_t>& a_dense, std::vector<uint8_t>& b_dense) {
    const uint32_t nv = sys.n_inputs + sys.n_aux;
    a_dense.assign(nv, 0);
    b_dense.assign(nv, 0);
    for (uint32_t i = 0; i < sys.n_inputs; i++) a_dense[i] = 1;
    for (uint32_t v : sys.m[0].col) a_dense[v] = 1;
    for (uint32_t v : sys.m[1].col) b_dense[v] = 1;
}

// ZKAMD_MERGE_VALUES=0: the maps are built without value pairs (a term per variable), for measurements and parity
bool merge_values_on() {
    const char* e = getenv("ZKAMD_MERGE_VALUES");
    return !(e && atoi(e) == 0);
}

// Build (or reuse) the per-circuit index maps from the density trackers.
// Equal points of a query (zk_params::Groups) become ONE term of its job: every member's slot maps to -1 and a slot appended
// for the group, whose scalar k_build_scalars makes the sum of the members', maps to the group's first point.
// ZKAMD_MERGE_BASES=0 builds the maps without groups (a term per query entry), for measurements and parity.
zk_status ensure_maps(zk_params* P, uint32_t n_in, uint32_t n_aux, const uint8_t* a_aux_d, const uint8_t* b_in_d,
                      const uint8_t* b_aux_d) {
    const char* merge_env = getenv("ZKAMD_MERGE_BASES");
    const bool merge = !(merge_env && atoi(merge_env) == 0);
    std::vector<uint8_t> key;
    key.reserve(9 + n_in + 2 * (size_t)n_aux);
    for (int i = 0; i < 4; i++) key.push_back((uint8_t)(n_in >> (8 * i)));
    for (int i = 0; i < 4; i++) key.push_back((uint8_t)(n_aux >> (8 * i)));
    key.insert(key.end(), a_aux_d, a_aux_d + n_aux);
    key.insert(key.end(), b_in_d, b_in_d + n_in);
    key.insert(key.end(), b_aux_d, b_aux_d + n_aux);
    for (int i = 0; i < 4; i++) key.push_back((uint8_t)((P->bind.drv.ready ? P->bind.drv.serial : 0u) >> (8 * i)));
    key.push_back(merge ? 1 : 0);
    const uint32_t nv = n_in + n_aux;
    // value pairs: over the derived set that carries them (its serial is in the key), unless ZKAMD_MERGE_VALUES=0
    const bool pairs = merge_values_on() && P->bind.drv.ready && P->bind.prs.ready && P->bind.prs.links.size() == 11 * (size_t)nv;
    key.push_back(pairs ? 1 : 0);
    if (key == P->maps.dens_key) return ZK_OK;
    const zk_params::Binding::Pairs& X = P->bind.prs;
    const PairCounts pc = pairs ? X.counts() : PairCounts();
    // scalar layout per proof: [inputs | aux | 1 | r | s | sums of the A groups | sums of the B2 groups] (prove_plan.h CJobLayout)
    const QueryPositions qp = query_positions(n_in, n_aux, a_aux_d, b_in_d, b_aux_d);
    // a different count means the assignment belongs to another circuit than the key
    if (qp.n_a() != P->key.n_a)
        return fail(ZK_ERR_IO, "the A density of the assignment (" + std::to_string(qp.n_a()) + ") differs from the key's a query (" +
                                   std::to_string(P->key.n_a) + ")");
    if (qp.n_b() != P->key.n_b1 || qp.n_b() != P->key.n_b2)
        return fail(ZK_ERR_IO, "the B density of the assignment (" + std::to_string(qp.n_b()) + ") differs from the key's b queries (" +
                                   std::to_string(P->key.n_b1) + " in G1, " + std::to_string(P->key.n_b2) + " in G2)");
    std::vector<int32_t> ma(qp.pos_a), mb1(qp.pos_b), mb2(qp.pos_b);
    for (std::vector<int32_t>* map : {&ma, &mb1, &mb2}) map->resize(nv + 3, -1);
    if (!P->key.alpha_g1_inf) ma[nv] = (int32_t)P->key.n_a;    // 1 * alpha_g1
    ma[nv + 1] = (int32_t)P->key.n_a + 1;                      // r * delta_g1 (never at infinity here: prove_* refuse)
    if (!P->key.beta_g1_inf) mb1[nv] = (int32_t)P->key.n_b1;   // 1 * beta_g1
    if (!P->key.beta_g2_inf) mb2[nv] = (int32_t)P->key.n_b2;   // 1 * beta_g2
    mb2[nv + 2] = (int32_t)P->key.n_b2 + 1;                    // s * delta_g2
    // the groups of each query: members muted in that query's map; base[g] = the query position the group's sum goes to;
    // the CSR lists in variable indices, A | B2 | B1, are what k_build_scalars sums over
    static const zk_params::Groups none;
    std::vector<uint32_t> gptr(1, 0u), gmem;
    auto mute = [&](const zk_params::Groups& G, const std::vector<uint32_t>& var, std::vector<int32_t>& map, std::vector<int32_t>& base) {
        for (uint32_t g = 0; g < G.count(); g++) {
            base.push_back((int32_t)G.mem[G.ptr[g]]);
            for (uint32_t k = G.ptr[g]; k < G.ptr[g + 1]; k++) {
                map[var[G.mem[k]]] = -1;
                gmem.push_back(var[G.mem[k]]);
            }
            gptr.push_back((uint32_t)gmem.size());
        }
    };
    std::vector<int32_t> base_a, base_b2, base_b1;
    mute(merge ? P->key.grp_a : none, qp.var_a, ma, base_a);
    mute(merge ? P->key.grp_b2 : none, qp.var_b, mb2, base_b2);
    mute(merge ? P->key.grp_b1 : none, qp.var_b, mb1, base_b1);
    const uint32_t ga = (uint32_t)base_a.size(), gb2 = (uint32_t)base_b2.size(), gb1 = (uint32_t)base_b1.size();
    // (each of the two jobs over this vector selects its own sums; the other's stay -1)
    const CJobLayout W = cjob_layout(n_in, n_aux, (uint32_t)P->key.m, ga, gb2, gb1, false, false);
    ma.resize(W.wstride, -1);
    mb2.resize(W.wstride, -1);
    for (uint32_t g = 0; g < ga; g++) ma[W.w_sum_a + g] = base_a[g];
    for (uint32_t g = 0; g < gb2; g++) mb2[W.w_sum_b2 + g] = base_b2[g];
    // h coefficients leave the last transform in bit-reversed order; the top coefficient
    // (degree m - 1) is dropped exactly as bellman truncates it
    std::vector<int32_t> mh(P->key.m);
    for (size_t pos = 0; pos < P->key.m; pos++) {
        uint32_t e = P->key.log_m ? (__builtin_bitreverse32((uint32_t)pos) >> (32 - P->key.log_m)) : 0;
        mh[pos] = e < P->key.n_h ? (int32_t)e : -1;
    }
    // The index map of the merged C job, absolute positions in the G1 group table, section by section where the layout has
    // them (prove_plan.h CJobLayout: what k_build_scalars stores by): the H block, the aux and - derived - the input variables
    // on the bases given, the r and fold sections and the sums of the groups on the copies of the b_g1 and A queries.
    auto upload_c_map = [&](DevBuf& dst, const CJobLayout& L, const int32_t* head, const int32_t* aux, const int32_t* inputs,
                            uint32_t off_a, uint32_t off_b1) -> zk_status {
        std::vector<int32_t> map(head, head + L.head);
        map.reserve(L.cstride);
        bool fits = true;
        auto section = [&](uint32_t off) { fits = fits && map.size() == off; };
        auto query = [&](const std::vector<int32_t>& q, uint32_t from, uint32_t n, uint32_t off) {
            for (uint32_t i = from; i < from + n; i++) map.push_back(q[i] < 0 ? -1 : (int32_t)(off + q[i]));
        };
        section(L.aux);
        map.insert(map.end(), aux, aux + n_aux);
        section(L.rz);
        query(mb1, 0, nv, off_b1);
        section(L.r);
        query(mb1, nv, 1, off_b1);   // r * beta_1
        if (L.fold) {   // [s z (nv) | s | r s] over the A query, alpha_1, delta_1
            section(L.sz);
            query(ma, 0, nv, off_a);
            section(L.s);
            query(ma, nv, 1, off_a);
            section(L.rs);
            query(ma, nv + 1, 1, off_a);
        }
        if (L.derived) {
            section(L.in_tail);
            map.insert(map.end(), inputs, inputs + n_in);
        }
        section(L.sum_b1);
        query(base_b1, 0, gb1, off_b1);
        if (L.fold) {
            section(L.sum_a);
            query(base_a, 0, ga, off_a);
        }
        if (L.w_b2v) {   // the pair bases lie in the table as the layout orders them (ensure_derived)
            for (Query qy : BOUND_G1_ORDER) {
                if (qy == QA && !L.fold) continue;
                section(qy == QL ? L.pair_l : qy == QB1 ? L.pair_b1 : L.pair_a);
                for (uint32_t k = 0; k < pc[qy]; k++) map.push_back((int32_t)(X.q[qy].base + k));
            }
        }
        section(L.cstride);
        if (!fits) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: the C map does not follow its layout");
        return dst.upload(map);
    };
    std::vector<int32_t> hk;   // the key's own bases: [h (m) | l (n_aux)]
    hk.reserve(P->key.m + n_aux);
    for (size_t pos = 0; pos < P->key.m; pos++) hk.push_back(mh[pos] < 0 ? -1 : (int32_t)(P->key.off_h + mh[pos]));
    for (uint32_t j = 0; j < n_aux; j++) hk.push_back((int32_t)(P->key.off_l + j));
    for (bool fold : {false, true})
        ZK_TRY(upload_c_map(fold ? P->maps.map_cf : P->maps.map_c, cjob_layout(n_in, n_aux, (uint32_t)P->key.m, ga, gb2, gb1, fold, false), hk.data(),
                            hk.data() + P->key.m, nullptr, P->key.off_a, P->key.off_b1));
    if (P->bind.drv.ready && P->bind.drv.pos.size() == 2 * (size_t)P->bind.drv.n_rows + nv) {
        // the same job over the derived bases, pos = [s (n_rows) | e (n_rows) | inputs | aux]
        const zk_params::Binding::Derived& D = P->bind.drv;
        const uint32_t head = 2 * D.n_rows;
        for (bool fold : {false, true})
            ZK_TRY(upload_c_map(fold ? P->maps.map_cfd : P->maps.map_cd, cjob_layout(n_in, n_aux, head, ga, gb2, gb1, fold, true, pc), D.pos.data(),
                                D.pos.data() + head + n_in, D.pos.data() + head, D.off_a, D.off_b1));
    }
    if (pairs) {
        // The A and B2 jobs of a chunk with pairs: the A map in absolute positions of the derived table (its copy of the A query,
        // the pair bases in front of it), the B2 map over its own copy of the variables' slots and the table with its pairs
        const CJobLayout Wp = cjob_layout(n_in, n_aux, 0, ga, gb2, gb1, false, true, pc);
        std::vector<int32_t> mad(Wp.wstride, -1), mbd(Wp.wstride, -1);
        for (uint32_t i = 0; i < W.wstride; i++) {
            if (ma[i] >= 0) mad[i] = (int32_t)(P->bind.drv.off_a + ma[i]);
            if (i >= nv) mbd[i] = mb2[i];
        }
        for (uint32_t i = 0; i < nv; i++) mbd[Wp.w_b2v + i] = mb2[i];
        for (uint32_t k = 0; k < pc.a; k++) mad[Wp.w_pair_a + k] = (int32_t)(X.q[QA].base + k);
        for (uint32_t k = 0; k < pc.b2; k++) mbd[Wp.w_pair_b2 + k] = (int32_t)(X.q[QB2].base + k);
        ZK_TRY(P->maps.map_ad.upload(mad));
        ZK_TRY(P->maps.map_b2d.upload(mbd));
        ZK_TRY(P->maps.pairs_dev.upload(X.links));
        // MsmSelRange::alt: per pair slot of the job, in the order of its sections, the table positions of the longer bases
        auto alts = [&](const auto& queries) {
            std::vector<int32_t> out;
            for (Query qy : queries)
                for (int32_t x : X.q[qy].alt) out.push_back(x < 0 ? -1 : (int32_t)(X.q[qy].xbase + (uint32_t)x));
            if (out.empty()) out.push_back(-1);
            return out;
        };
        if (zkpairs::RUN_MAX > 2) {
            const Query a_alone[1] = {QA};
            ZK_TRY(P->maps.alt_c.upload(alts(BOUND_G1_ORDER)));   // [pl | pb1 | (fold: pa)]
            ZK_TRY(P->maps.alt_a.upload(alts(a_alone)));
            ZK_TRY(P->maps.alt_b2.upload(alts(BOUND_G2_ORDER)));
        }
    }
    gptr.insert(gptr.end(), gmem.begin(), gmem.end());
    ZK_TRY(P->maps.grp_dev.upload(gptr));
    ZK_TRY(P->maps.map_a.upload(ma));
    ZK_TRY(P->maps.map_b2.upload(mb2));
    P->maps.dens_key.swap(key);
    P->maps.map_nv = nv;
    P->maps.mg_a = ga;
    P->maps.mg_b2 = gb2;
    P->maps.mg_b1 = gb1;
    P->maps.mpairs = pc;
    return ZK_OK;
}


// ------------------------------------------------------------------------------------------
// Derived bases of a (key, circuit) pair: four transforms per proof instead of six, H scalars on the live rows only
// ------------------------------------------------------------------------------------------
// With p = a b - c = q Z + R (Z = x^m - 1, deg R < m), bellman's h is q + R / (g^m - 1): q is the quotient and R = sum_k e_k L_k
// interpolates the residuals e_k = a_k b_k - c_k of the rows, for ANY a, b, c; bellman drops h_(m-1).  On the DOMAIN
//     q(w^j) = (a b - W)'(w^j) w^j / m,        W = the interpolant of the row products w_k = c_k + e_k
// (differentiate p - R = q Z at a root of Z).  Its a b part is s_j / m with s_j = da_j b_j + a_j db_j, da_j = w^j a'(w^j) =
// sum_t t a_t w^(jt): one plain forward transform of the coefficients times their index.  Its W part is LINEAR in w, and so
// is R: both transpose onto the bases once.  With H'_t = H_t, H'_(m-1) := the identity (the truncation),
//     Lambda_k = (1/m) sum_t w^-kt H'_t,      M_k = -(1/m^2) sum_t t w^-kt H'_t
// - two inverse transforms "in the exponent" - and c_k = sum_i C_ki z_i the library's own row evaluations (k_r1cs_eval),
//     sum_t h_t H_t = sum_j s_j (Lambda_j / m) + sum_i z_i (sum_k C_ki M_k) + sum_k e_k (M_k + Lambda_k / (g^m - 1)).
// A padding row j >= n_rows = n_con + n_in has a_j = b_j = c_j = 0 for every assignment, so s_j = e_j = 0: the job has
// n_rows H scalars of full width (of m), n_rows residuals that are zero - no digits, no pairs - unless a constraint fails,
// and the variables' terms it had anyway:
//     C' = sum_j s_j Lambda_j / m + sum_k e_k E_k + sum_aux z_i (L_i + D_i) + sum_inputs z_i D_i + r (beta_1 + sum B1).
// Exact for every assignment, satisfying or not; nothing assumes that Z divides a b - c.
//
// Built on the GPU, one row of lanes per point (coop_tail.h basis_*): a scaling pass and log2 m butterfly stages per
// transform, every butterfly one 255-bit scalar product; D_i as one scalar product per entry of C summed per column, E_k
// as one per live row.  The set goes through into_affine and its own table of doublings, under the recoding width of its
// own term count; a base that comes out as the identity - D_i of an input that C never mentions - is mapped out like an
// identity in a key file.  Nothing happens when the pair cannot have one (a lane's clone, another circuit's shape): the
// caller then keeps the six-transform form.
// The value pairs of a (key, circuit) pair (value_pairs.h): for every link (p, j) of the circuit's chains and every query in
// which both variables have a term - dense there, the base not the identity - one more base P_j + P_p.  A member of a group
// of equal bases takes part with its own point, which is the group's: k_build_scalars leaves it out of the group's sum when
// its term goes into a pair.  set = the derived set [Lambda | E | D] in host form (the L terms of the job are its D block).  The
// sums are made on the host cores from the key's encodings; a sum that comes out as the identity has no base (both keep
// their terms).  Fills P->bind.prs but for where the bases lie; a circuit without built-in probes has no pairs.
// the natively emitted constraint systems of the two built-in circuits (transfer_r1cs.h), each built once per process
const zkr1cs::System& builtin_system(zkpairs::Circuit c) {
    if (c == zkpairs::TRANSFER) {
        static const zkr1cs::System sys = zkr1cs::transfer_system();
        return sys;
    }
    static const zkr1cs::System sys = zkr1cs::anonymous_system();
    return sys;
}
// the bases one group's queries get for their pairs and for their longer runs (value_pairs.h RUN_MAX), by query
template <class A>
struct QueryBases {
    std::vector<A> pairs[zkpairs::N_QUERIES], runs[zkpairs::N_QUERIES];
};
struct PairBases {
    QueryBases<HG1A> g1;
    QueryBases<HG2A> g2;
    std::vector<HG2A> b2;   // the b_g2 query as decoded for them: the head of the table its pairs lie in
};
// fn(k) for every k of [0, n) on the host threads, 64 and more to a thread
template <class Fn>
void spread(size_t n, Fn&& fn) {
    const unsigned nt = host_threads(n / 64 + 1, 32);
    auto part = [&](unsigned t) {
        for (size_t k = n * t / nt; k < n * (t + 1) / nt; k++) fn(k);
    };
    run_threads(nt, part);
}
// a query's points from its uncompressed encodings (n x sizeof(A) bytes); false when one is refused
template <class A, class Dec>
bool decode_query(const std::vector<uint8_t>& enc, Dec&& dec, std::vector<A>& out) {
    static_assert(sizeof(A) == 96 || sizeof(A) == 192, "an affine point in the host's layout is its uncompressed encoding's size");
    out.assign(enc.size() / sizeof(A), A::inf());
    std::atomic<bool> ok{true};
    spread(out.size(), [&](size_t i) {
        if (dec(enc.data() + i * sizeof(A), &out[i]) != zkhost::DEC_OK) ok = false;
    });
    return ok;
}
// One query's share of derived_pairs.  pos[v] = where the point of variable v's term lies in pts, -1 where it has none;
// chains, probes: of the circuit.  Fills the query's q array and its byte of the availability words in X.links, X.q[qy] but for
// where the bases lie, and the bases themselves.
template <class A>
void query_pairs(zk_params::Binding::Pairs& X, Query qy, const std::vector<int32_t>& chains, const std::vector<std::vector<Fr>>& probes,
                 const std::vector<int32_t>& pos, const std::vector<A>& pts, QueryBases<A>& out) {
    typedef zkhost::Point<decltype(A().x)> Pt;
    constexpr uint32_t W = zkpairs::RUN_MAX - 2;
    const size_t nv = pos.size();
    const int32_t* pred = chains.data() + 2 * nv * (size_t)zkpairs::chain_of(qy);
    int32_t* const q = &X.links[(6 + (size_t)qy) * nv];
    int32_t* const avail = &X.links[10 * nv];
    zk_params::Binding::Pairs::PerQuery& Q = X.q[qy];
    std::vector<A>& pairs = out.pairs[qy];
    std::vector<A>& runs = out.runs[qy];
    auto point = [&](int32_t v) { return Pt::from_affine(pts[pos[v]]); };
    // the links whose two ends both have a term, and the sums of their bases
    std::vector<uint32_t> js;
    for (uint32_t j = 0; j < nv; j++)
        if (pred[j] >= 0 && pos[j] >= 0 && pos[pred[j]] >= 0) js.push_back(j);
    std::vector<A> sums(js.size());
    spread(js.size(), [&](size_t k) { sums[k] = zkhost::to_affine(zkhost::padd(point(pred[js[k]]), point((int32_t)js[k]))); });
    for (size_t k = 0; k < js.size(); k++)
        if (!sums[k].is_inf()) {
            q[js[k]] = (int32_t)pairs.size();
            pairs.push_back(sums[k]);
        }
    Q.n = (uint32_t)pairs.size();
    // The longer runs: for every link j that has its pair base and l = 3 ... RUN_MAX, the sum of the l chain members that end at
    // j, as long as the links behind it have their pair bases.  The thread of j walks back from j, adding one member per length
    // (so P_j + P_pred is added again, per link) and normalises every length it keeps (an inversion each): 49 ms of binding for
    // the transfer key at 4.  A sum that comes out as the identity has no base and no bit: k_build_scalars then splits the run
    // into shorter terms.
    Q.alt.assign((size_t)Q.n * W, -1);
    if (W) {
        js.clear();
        for (uint32_t j = 0; j < nv; j++)
            if (q[j] >= 0 && q[pred[j]] >= 0) js.push_back(j);
        sums.assign(js.size() * W, A::inf());
        spread(js.size(), [&](size_t k) {
            const uint32_t j = js[k];
            int32_t cur = pred[j];
            auto acc = zkhost::padd(point((int32_t)j), point(cur));
            for (uint32_t l = 3; l <= zkpairs::RUN_MAX && q[cur] >= 0; l++) {
                cur = pred[cur];
                acc = zkhost::padd(acc, point(cur));
                sums[k * W + (l - 3)] = zkhost::to_affine(acc);
            }
        });
        for (size_t k = 0; k < js.size(); k++)
            for (uint32_t l = 3; l <= zkpairs::RUN_MAX; l++)
                if (!sums[k * W + (l - 3)].is_inf()) {
                    Q.alt[(size_t)q[js[k]] * W + (l - 3)] = (int32_t)runs.size();
                    runs.push_back(sums[k * W + (l - 3)]);
                    avail[js[k]] |= (int32_t)(1u << (8 * (uint32_t)qy + (l - 1)));
                    Q.xn[l - 3]++;
                }
    }
    // what a proof is expected to merge, from the probes
    uint64_t merged = 0;
    for (const std::vector<Fr>& z : probes) merged += zkpairs::count_merges(pred, pred + nv, q, avail, (uint32_t)qy, z);
    Q.expect = (uint32_t)(merged / probes.size());
}
zk_status derived_pairs(zk_params* P, const zk_r1cs* R, const std::vector<HG1A>& set, uint32_t n_rows, PairBases& out) {
    zk_params::Binding::Pairs& X = P->bind.prs;
    X = zk_params::Binding::Pairs();
    const uint32_t n_in = R->sys.n_in, n_aux = R->sys.n_aux, nv = n_in + n_aux;
    zkpairs::Circuit kind;
    if (n_in == ZK_TRANSFER_N_INPUTS && n_aux == ZK_TRANSFER_N_AUX) kind = zkpairs::TRANSFER;
    else if (n_in == ZK_ANONYMOUS_N_INPUTS && n_aux == ZK_ANONYMOUS_N_AUX) kind = zkpairs::ANONYMOUS;
    else return ZK_OK;
    const zk_params::Key& K = P->key;
    if (P->enc_a.size() != (size_t)K.n_a * 96 || P->enc_b1.size() != (size_t)K.n_b1 * 96 || P->enc_b2.size() != (size_t)K.n_b2 * 192) return ZK_OK;
    const QueryPositions qp = query_positions(n_in, n_aux, R->sys.a_aux_density.data(), R->sys.b_input_density.data(), R->sys.b_aux_density.data());
    if (qp.n_a() != K.n_a || qp.n_b() != K.n_b1 || qp.n_b() != K.n_b2) return ZK_OK;
    std::vector<uint8_t> a_dense(nv), b_dense(nv);
    for (uint32_t i = 0; i < nv; i++) {
        a_dense[i] = qp.pos_a[i] >= 0;
        b_dense[i] = qp.pos_b[i] >= 0;
    }
    {
        // The probes are witnesses of the BUILT-IN circuit: another circuit with its counts would get chains that merge nothing
        // and pay for their bases and tables.  The caller's matrices must have the built-in system's constraint count and
        // densities (which variables occur in A and in B) - what the chains are made from.
        const zkr1cs::System& sys = builtin_system(kind);
        if (sys.n_inputs != n_in || sys.n_aux != n_aux || sys.n_constraints != R->sys.n_con) return ZK_OK;
        std::vector<uint8_t> sa, sb;
        system_densities(sys, sa, sb);
        if (sa != a_dense || sb != b_dense) return ZK_OK;
    }
    const std::vector<std::vector<Fr>>& probes = zkpairs::circuit_probes(kind);
    if (probes.empty() || probes[0].size() != nv || set.size() != 2 * (size_t)n_rows + nv) return ZK_OK;
    // [pred A | succ A | pred B | succ B | pred L | succ L]
    const std::vector<int32_t> chains = zkpairs::chains_of(probes, n_in, a_dense, b_dense);
    // the L terms of the job are the D block of the set: an aux variable has one where its base is not the identity
    std::vector<int32_t> pos_l(nv, -1);
    for (uint32_t i = n_in; i < nv; i++)
        if (!set[2 * (size_t)n_rows + i].is_inf()) pos_l[i] = (int32_t)(2 * n_rows + i);
    // the points of the three queries, decoded from the key's encodings a second time (the load decoded them on the device)
    std::vector<HG1A> pts_a, pts_b1;
    const bool decoded = decode_query(P->enc_a, zkhost::g1_from_uncompressed, pts_a) && decode_query(P->enc_b1, zkhost::g1_from_uncompressed, pts_b1) &&
                         decode_query(P->enc_b2, zkhost::g2_from_uncompressed, out.b2);
    if (!decoded) return fail(ZK_ERR_IO, "internal: a query of the key does not decode a second time");
    // links = [the chains | qa | qb2 | ql | qb1 | the bits of the longer bases]
    X.links.assign(11 * (size_t)nv, -1);
    std::copy(chains.begin(), chains.end(), X.links.begin());
    std::fill(X.links.begin() + 10 * (size_t)nv, X.links.end(), 0);
    query_pairs(X, QA, chains, probes, qp.pos_a, pts_a, out.g1);
    query_pairs(X, QB2, chains, probes, qp.pos_b, out.b2, out.g2);
    query_pairs(X, QL, chains, probes, pos_l, set, out.g1);
    query_pairs(X, QB1, chains, probes, qp.pos_b, pts_b1, out.g1);
    X.ready = X.counts().any();
    return ZK_OK;
}

// ZKAMD_TABLE_MULTIPLES = 1 | 2 | 4 | 8: the odd multiples of every slice the bound tables carry (msm_types.h MsmRecode).  Table memory
// and bind time grow with it, the (digit, point) pairs of every full-width scalar shrink.  The key's own tables keep one.
// A key carries them from its first launch set of ZKAMD_TABLE_MULTIPLES_MIN jobs on (default 129: the batch form of a set) or
// from the pipeline made over it: a proof made alone binds the key as fast as it did and holds no larger tables.
#ifndef ZK_TABLE_MULTIPLES_DEFAULT
#define ZK_TABLE_MULTIPLES_DEFAULT 8
#endif
uint32_t table_multiples() {
    const char* env = getenv("ZKAMD_TABLE_MULTIPLES");
    const int v = env ? atoi(env) : 0;
    return v == 1 || v == 2 || v == 4 || v == 8 ? (uint32_t)v : ZK_TABLE_MULTIPLES_DEFAULT;
}
size_t table_multiples_min() {
    const char* env = getenv("ZKAMD_TABLE_MULTIPLES_MIN");
    return env && atol(env) > 0 ? (size_t)atol(env) : 129;
}

// The multiples of the two bound tables, once per binding, when its first batch arrives.  A table that does not fit stays as it
// is (each table recodes by what it holds); the host trace says what was taken.
zk_status add_table_multiples(zk_params* P) {
    zk_params::Binding& B = P->bind;
    const uint32_t asked = table_multiples();
    if (B.drv.multiples_tried || !B.g1d.table.owned) return ZK_OK;
    B.drv.multiples_tried = true;
    if (asked <= 1) return ZK_OK;
    ZK_TRY(use_device(P->key.device));
    const auto t0 = std::chrono::steady_clock::now();
    zk_status st = hook_env("ZKAMD_INJECT_TABLE_OOM") ? fail(ZK_ERR_OUT_OF_MEMORY, "injected: the table with its multiples does not fit")
                                                     : B.g1d.add_multiples(asked);
    if (st == ZK_OK && B.prs.ready) st = B.g2p.add_multiples(asked);
    if (st != ZK_OK && st != ZK_ERR_OUT_OF_MEMORY) return st;
    B.g1d_lone.alias(B.g1d, B.g1d_lone.c);
    if (B.prs.ready) {
        B.g1da.alias(B.g1d, B.g1da.c);
        B.g2p_lone.alias(B.g2p, B.g2p_lone.c);
    }
    if (getenv("ZKAMD_TRACE_HOST"))
        fprintf(stderr, "[zkamd] table multiples: %u asked%s, G1 table %u per slice %.2f GB, G2 table %u per slice %.2f GB, %.1f ms\n", asked,
                st == ZK_OK ? "" : " (out of memory)", B.g1d.n_mult, (double)B.g1d.bytes / 1e9, B.g2p.n_mult, (double)B.g2p.bytes / 1e9,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return ZK_OK;
}

// batch: the caller has a launch set of table_multiples_min() jobs or more, or is making a pipeline
zk_status ensure_derived(zk_params* P, zk_r1cs* R, bool batch) {
    if (P->bind.drv.ready && P->bind.drv.circuit == R->sys.id) return batch ? add_table_multiples(P) : ZK_OK;
    P->bind.drv.multiples_tried = false;
    const uint32_t n_in = R->sys.n_in, n_aux = R->sys.n_aux, nv = n_in + n_aux, n_con = R->sys.n_con, n_rows = n_con + n_in, k = P->key.log_m;
    const size_t m = P->key.m;
    if (!P->tab.g1.table.owned || R->sys.h_row_ptr[2].size() != (size_t)n_con + 1 || n_in != P->key.n_ic || n_aux != P->key.n_l ||
        (size_t)n_con + n_in > m || P->key.n_h + 1 != m)
        return ZK_OK;
    ZK_TRY(use_device(P->key.device));
    const auto t0 = std::chrono::steady_clock::now();
    typedef zkdev::XYZZ<zkdev::Fq> DP;
    typedef zkdev::Affine<zkdev::Fq> DA;
    P->bind.drv.ready = false;
    const DA* key = P->tab.g1.table.as<DA>();
    // C by columns, the coefficients in plain words
    const std::vector<uint32_t>& rp = R->sys.h_row_ptr[2];
    const std::vector<uint32_t>& cl = R->sys.h_col[2];
    const uint32_t nnz = rp[n_con];
    std::vector<uint32_t> ptr(nv + 1, 0), t_row(nnz ? nnz : 1), each(n_rows + 1);
    std::vector<Fr> t_s(nnz ? nnz : 1);
    for (uint32_t e = 0; e < nnz; e++) ptr[cl[e] + 1]++;
    for (uint32_t i = 0; i < nv; i++) ptr[i + 1] += ptr[i];
    {
        std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
        for (uint32_t row = 0; row < n_con; row++)
            for (uint32_t e = rp[row]; e < rp[row + 1]; e++) {
                const uint32_t slot = at[cl[e]]++;
                t_row[slot] = row;
                t_s[slot] = R->sys.h_coeff[2][e].from_mont();
            }
    }
    for (uint32_t i = 0; i <= n_rows; i++) each[i] = i;   // (segments of one term: E_k = M_k + one point)
    // H in bit-reversed order with the identity in the place of H_(m-1); the L query behind the (empty) inputs
    std::vector<int32_t> idx(m + nv);
    for (size_t pos = 0; pos < m; pos++) {
        const uint32_t e = k ? (__builtin_bitreverse32((uint32_t)pos) >> (32 - k)) : 0;
        idx[pos] = e < P->key.n_h ? (int32_t)(P->key.off_h + e) : -1;
    }
    for (uint32_t i = 0; i < nv; i++) idx[m + i] = i < n_in ? -1 : (int32_t)(P->key.off_l + (i - n_in));
    const size_t rows = std::max<size_t>(m, nnz), n_set = 2 * (size_t)n_rows + nv;
    DevBuf d_idx, d_ptr, d_each, d_row, d_s, d_tw, d_w, d_sl, d_sm, d_se, src, ping, pong, lam, mk, terms, tbl, all, stage;
    for (DevBuf* b : {&d_idx, &d_ptr, &d_each, &d_row, &d_s, &d_tw, &d_w, &d_sl, &d_sm, &d_se, &src, &ping, &pong, &lam, &mk, &terms, &tbl, &all, &stage})
        b->is_public = true;
    const Fr ninv2 = P->tab.ntt.n_inv * P->tab.ntt.n_inv;
    const Fr wv[5] = {P->tab.ntt.w_inv, Fr::one(), ninv2, -ninv2, fr_from_u64((uint64_t)m) * P->tab.ntt.z_inv};
    ZK_TRY(d_idx.upload(idx));
    ZK_TRY(d_ptr.upload(ptr));
    ZK_TRY(d_each.upload(each));
    ZK_TRY(d_row.upload(t_row));
    ZK_TRY(d_s.upload(t_s));
    ZK_TRY(d_w.upload(wv, 5));
    ZK_TRY(d_tw.ensure(m * 32));
    ZK_TRY(d_sl.ensure(m * 32));
    ZK_TRY(d_sm.ensure(m * 32));
    ZK_TRY(d_se.ensure((size_t)n_rows * 32));
    ZK_TRY(src.ensure((m + nv) * sizeof(DP)));
    ZK_TRY(ping.ensure(m * sizeof(DP)));
    ZK_TRY(pong.ensure(m * sizeof(DP)));
    ZK_TRY(lam.ensure(m * sizeof(DP)));
    ZK_TRY(mk.ensure(m * sizeof(DP)));
    ZK_TRY(terms.ensure(std::max<size_t>(nnz ? nnz : 1, n_rows) * sizeof(DP)));
    ZK_TRY(tbl.ensure(15 * rows * sizeof(DP)));
    ZK_TRY(all.ensure(n_set * sizeof(DP)));
    const uint32_t* cw = d_w.as<uint32_t>();
    auto table = [&](DevBuf& out, const uint32_t* base, const uint32_t* scale, uint32_t mode, size_t count) {
        ZK_LAUNCH(zkdev::k_fr_pow_table, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, g_stream, out.as<uint32_t>(), base, scale,
                  k, mode, 1u, (uint32_t)count);
    };
    // plain words: w^-e for e < m / 2; 1 / m^2 and - t / m^2 at the bit-reversed position of t; m / (g^m - 1) per live row
    if (m > 1) table(d_tw, cw, cw + 8, 0, m / 2);
    table(d_sl, cw + 8, cw + 16, 2, m);
    table(d_sm, cw + 8, cw + 24, 3, m);
    table(d_se, cw + 8, cw + 32, 2, n_rows);
    zkcoop::basis_gather(key, d_idx.as<int32_t>(), src.as<DP>(), (uint32_t)(m + nv), g_stream);
    // in: the scaled points in bit-reversed order; out: the transform in natural order
    auto transform = [&](const uint32_t* scale, DP* out) -> zk_status {
        DP *a = ping.as<DP>(), *b = pong.as<DP>();
        zkcoop::basis_scale(src.as<DP>(), nullptr, scale, tbl.as<DP>(), k ? a : out, (uint32_t)m, g_stream);
        for (uint32_t st = 0; st < k; st++) {
            zkcoop::basis_dft_stage(a, st + 1 == k ? out : b, d_tw.as<uint32_t>(), tbl.as<DP>(), k, st, g_stream);
            std::swap(a, b);
        }
        HIP_TRY(hipGetLastError());
        return ZK_OK;
    };
    ZK_TRY(transform(d_sl.as<uint32_t>(), lam.as<DP>()));   // Lambda_j / m: the 1 / m of s_j rides in the base
    ZK_TRY(transform(d_sm.as<uint32_t>(), mk.as<DP>()));    // M_k
    DP* set = all.as<DP>();
    HIP_TRY(hipMemcpyAsync(set, lam.p, (size_t)n_rows * sizeof(DP), hipMemcpyDeviceToDevice, g_stream));
    // E_k = M_k + (m / (g^m - 1)) (Lambda_k / m)
    zkcoop::basis_scale(lam.as<DP>(), nullptr, d_se.as<uint32_t>(), tbl.as<DP>(), terms.as<DP>(), n_rows, g_stream);
    zkcoop::basis_segment_sums(mk.as<DP>(), terms.as<DP>(), d_each.as<uint32_t>(), set + n_rows, n_rows, g_stream);
    // D_i = sum_k C_ki M_k, behind L_i for an aux variable
    if (nnz) zkcoop::basis_scale(mk.as<DP>(), d_row.as<uint32_t>(), d_s.as<uint32_t>(), tbl.as<DP>(), terms.as<DP>(), nnz, g_stream);
    zkcoop::basis_segment_sums(src.as<DP>() + m, terms.as<DP>(), d_ptr.as<uint32_t>(), set + 2 * (size_t)n_rows, nv, g_stream);
    HIP_TRY(hipGetLastError());
    std::vector<HG1> host(n_set);
    ZK_TRY(P->tab.g1.normalize_to_host(set, n_set, host.data(), stage, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    std::vector<HG1A> pts(n_set);
    P->bind.drv.pos.assign(n_set, -1);
    size_t live = 0;
    for (size_t i = 0; i < n_set; i++) {
        pts[i] = host[i].is_inf() ? HG1A::inf() : HG1A{host[i].x, host[i].y};
        if (!host[i].is_inf()) {
            P->bind.drv.pos[i] = (int32_t)i;
            if (i < n_rows || i >= 2 * (size_t)n_rows) live++;
        }
    }
    // (the width of the set's own terms: the residuals are zero scalars unless a constraint fails)
    // value pairs: [pairs of the L terms | of the B1 query | of the A query] behind the set, the B2 query's in a table of its own.
    // A set expects fewer terms per proof with them (the mean over the probes), and its width follows that.
    PairBases pb;
    ZK_TRY(derived_pairs(P, R, pts, n_rows, pb));
    zk_params::Binding::Pairs& X = P->bind.prs;
    // the pair sections in the order of the table, then the longer runs' behind all of them, each noted where it begins
    auto append = [&X](auto& table, const auto& bases, const auto& order) {
        for (Query qy : order) {
            X.q[qy].base = (uint32_t)table.size();
            table.insert(table.end(), bases.pairs[qy].begin(), bases.pairs[qy].end());
        }
        for (Query qy : order) {
            X.q[qy].xbase = (uint32_t)table.size();
            table.insert(table.end(), bases.runs[qy].begin(), bases.runs[qy].end());
        }
    };
    append(pts, pb.g1, BOUND_G1_ORDER);
#ifdef ZK_TEST_HOOKS
    X.hook_g1.assign(pts.begin() + X.q[BOUND_G1_ORDER[0]].xbase, pts.end());
    X.hook_d.assign(pts.begin() + 2 * (size_t)n_rows, pts.begin() + 2 * (size_t)n_rows + nv);
#endif
    const zk_params::Key& K = P->key;
    const bool values = merge_values_on();   // (the widths of a run with the switch off stay those of a set without pairs)
    std::vector<HG2A> pts2;
    if (X.ready) {
        pts2.swap(pb.b2);
        pts2.resize(K.n_b2 + 2, HG2A::inf());
        if (K.vk_bytes.size() < 864 || zkhost::g2_from_uncompressed(K.vk_bytes.data() + 192, &pts2[K.n_b2]) != zkhost::DEC_OK ||
            zkhost::g2_from_uncompressed(K.vk_bytes.data() + 672, &pts2[K.n_b2 + 1]) != zkhost::DEC_OK)
            return fail(ZK_ERR_IO, "internal: beta_2 and delta_2 do not decode a second time");
        append(pts2, pb.g2, BOUND_G2_ORDER);
#ifdef ZK_TEST_HOOKS
        X.hook_g2.assign(pts2.begin() + X.q[BOUND_G2_ORDER[0]].xbase, pts2.end());
#endif
    }
    // The two bound tables, as they were: the odd multiples of their slices (msm_types.h MsmRecode) come with the first batch
    // (add_table_multiples), and the widths stay those of one multiple (msm_group.h pick_window).
    const uint32_t c_set = pick_window(live + K.n_b1 - (values ? std::min<size_t>(X.q[QL].expect + X.q[QB1].expect, live) : 0), 1);
    ZK_TRY(P->bind.g1d.build_with_tail(pts, P->tab.g1, K.off_a, P->tab.g1.n_points - K.off_a, c_set));
    P->bind.g1d_lone.alias(P->bind.g1d, P->tab.g1_lone.c);
    if (X.ready) {
        P->bind.g1da.alias(P->bind.g1d, values ? pick_window(K.n_a - std::min(X.q[QA].expect, K.n_a), 3) : P->tab.g1a.c);
        const uint32_t c2 = values ? pick_window(K.n_b2 - std::min(X.q[QB2].expect, K.n_b2), 2) : P->tab.g2.c;
        ZK_TRY(P->bind.g2p.build(pts2, c2, false, "pair bases (G2)"));
        P->bind.g2p_lone.alias(P->bind.g2p, getenv("ZKAMD_WINDOW_BITS_G2") || c2 <= 10 ? c2 : 10u);
    }
    P->bind.drv.n_rows = n_rows;
    P->bind.drv.off_a = (uint32_t)pts.size();
    P->bind.drv.off_b1 = P->bind.drv.off_a + P->key.n_a + 2;
    P->bind.drv.circuit = R->sys.id;
    static std::atomic<uint32_t> serial{1};
    P->bind.drv.serial = serial++;
    P->bind.drv.bind_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    P->bind.drv.ready = true;
    if (getenv("ZKAMD_TRACE_HOST"))
        fprintf(stderr, "[zkamd] derived bases: 2 x %u + %u points, %u entries of C, width %u, %.1f ms, table %.2f GB\n", n_rows, nv, nnz,
                c_set, P->bind.drv.bind_ms, (double)P->bind.g1d.bytes / 1e9);
    if (getenv("ZKAMD_TRACE_HOST") && X.ready)
        fprintf(stderr, "[zkamd] value pairs: bases a %u, b_g2 %u, l %u, b_g1 %u; merges expected per proof %u, %u, %u, %u; widths "
                        "C' %u, A %u, G2 %u; G2 table %.2f GB\n", X.q[QA].n, X.q[QB2].n, X.q[QL].n, X.q[QB1].n, X.q[QA].expect, X.q[QB2].expect, X.q[QL].expect, X.q[QB1].expect,
                c_set, P->bind.g1da.c, P->bind.g2p.c, (double)P->bind.g2p.bytes / 1e9);
    if (getenv("ZKAMD_TRACE_HOST") && X.ready)
        for (uint32_t l = 3; l <= zkpairs::RUN_MAX; l++)
            fprintf(stderr, "[zkamd] value runs: bases of %u members: a %u, b_g2 %u, l %u, b_g1 %u\n", l, X.q[QA].xn[l - 3], X.q[QB2].xn[l - 3],
                    X.q[QL].xn[l - 3], X.q[QB1].xn[l - 3]);
    return batch ? add_table_multiples(P) : ZK_OK;
}

}  // namespace
