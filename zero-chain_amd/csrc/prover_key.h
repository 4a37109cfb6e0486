// The proving key handle (zk_params) as the parts it is made of, each with one rule for how another lane of a pipeline gets it:
//   Key      what the parameter file says (plain data)                     copied
//   Tables   the NTT plan and the five MSM groups over the key's bases     shared (borrowed tables, own workspaces)
//   Binding  what ensure_derived builds for one (key, circuit) pair        shared
//   Maps     the cache of ensure_maps for one density pattern              the handle's own
//   Work     the workspaces of a chunk                                     the handle's own
// and params_load with its readers, and the two lane clones.  Included by zkamd.cpp alone: its kernels are compiled there.
#pragma once
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include "../../include/zkamd.h"
#include "gpu_rt.h"
#include "host_common.h"
#include "host_math.h"
#include "ntt.h"
#include "ntt_plan.h"
#include "msm_group.h"
#include "prove_plan.h"
#include "transfer_witness.h"
#include "value_pairs.h"
#include "handles.h"
#include "transfer_r1cs.h"

using zkdev::MsmJob;
using zkdev::NttPass;

namespace {

using namespace zkrt;

// ------------------------------------------------------------------------------------------
// NTT plan: twiddles and fused scaling tables for one domain size, resident in HBM
// ------------------------------------------------------------------------------------------
using zkhost::Fr;

Fr fr_from_u64(uint64_t v) {
    Fr x = Fr::zero();
    x.l[0] = v;
    return x.to_mont();
}
Fr fr_const(const uint64_t (&v)[4]) {
    Fr x;
    for (int i = 0; i < 4; i++) x.l[i] = v[i];
    return x;
}


struct NttPlan {
    uint32_t log_n = 0;
    size_t n = 0;
    DevBuf tw_fwd, tw_inv;           // w^e, w^-e, e < n/2 (Montgomery)
    DevBuf s1_plain, s1_mont, s2;    // prover tables, bit-reversed order (see prove_chunk)
    DevBuf sc_plain, sc_mont;        // constant 1 / (n (g^n - 1)): the scaling of c's coefficients (k_h_pointwise)
    DevBuf coset_fwd, coset_inv;     // g^i and g^-i / n, natural order (Montgomery)
    DevBuf dt;                       // t / n at the bit-reversed position of t (Montgomery): a's coefficients -> those of x a'(x)
    DevBuf consts;                   // [0] = 1/n, [1] = 1/(g^n - 1)   (Montgomery)
    Fr w_inv, n_inv, z_inv;          // w^-1, 1/n, 1/(g^n - 1) (Montgomery): the transforms of the derived bases make their own tables
    DevBuf scratch;                  // permutation scratch for the stand-alone entry
    size_t bytes = 0;

    // The tile choice of the transforms of 2^17 and more, read once per process (ZKAMD_NTT_TILES, ntt_plan.h ntt_tiles), and the
    // form of a chain of `batch` transforms of this size under it: the product's one place that decides a form.
    static NttForm tiles() {
        static const NttForm f = ntt_tiles(getenv("ZKAMD_NTT_TILES"));
        return f;
    }
    NttForm form(uint32_t batch) const { return ntt_form(tiles(), log_n, batch); }

    // Another lane's view of the same plan: the tables borrowed, the scalars copied; o must outlive it.  (scratch is the stand-alone
    // entry's workspace, and bytes accounts for the owner's tables: neither is shared.)
    void share(const NttPlan& o) {
        log_n = o.log_n;
        n = o.n;
        w_inv = o.w_inv;
        n_inv = o.n_inv;
        z_inv = o.z_inv;
        DevBuf NttPlan::*const tables[] = {&NttPlan::tw_fwd, &NttPlan::tw_inv, &NttPlan::s1_plain, &NttPlan::s1_mont, &NttPlan::s2, &NttPlan::sc_plain,
                                           &NttPlan::sc_mont, &NttPlan::coset_fwd, &NttPlan::coset_inv, &NttPlan::dt, &NttPlan::consts};
        for (DevBuf NttPlan::*t : tables) (this->*t).borrow(o.*t);
    }

    zk_status pow_table(DevBuf& out, const Fr& base, const Fr& scale, uint32_t mode, uint32_t raw, size_t count) {
        DevBuf tmp;
        Fr bs[2] = {base, scale};
        ZK_TRY(tmp.upload(bs, 2));
        ZK_TRY(out.ensure(count * 32));
        bytes += count * 32;
        if (count == 0) return ZK_OK;
        ZK_LAUNCH(zkdev::k_fr_pow_table, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, g_stream,
                  out.as<uint32_t>(), tmp.as<uint32_t>(), tmp.as<uint32_t>() + 8, log_n, mode, raw, (uint32_t)count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g_stream));
        return ZK_OK;
    }

    zk_status init(uint32_t k) {
        if (k > 27) return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "domain larger than 2^27");
        log_n = k;
        n = (size_t)1 << k;
        static const uint64_t root_v[4] = ZK_FR_ROOT_OF_UNITY_MONT_64;
        static const uint64_t gen_v[4] = ZK_FR_GENERATOR_MONT_64;
        static const uint64_t r2_v[4] = ZK_FR_R2_64;
        Fr w = fr_const(root_v);
        for (uint32_t i = k; i < ZK_FR_S; i++) w = w.sqr();   // w = ROOT^(2^(S-k))  (domain.rs)
        Fr winv = zkhost::fr_inv(w);
        Fr g = fr_const(gen_v), ginv = zkhost::fr_inv(g);
        Fr ninv = zkhost::fr_inv(fr_from_u64((uint64_t)n));
        Fr r_elem = fr_const(r2_v);   // Montgomery form of the field element R
        Fr gn = g;
        for (uint32_t i = 0; i < k; i++) gn = gn.sqr();
        Fr zinv = zkhost::fr_inv(gn - Fr::one());   // divide_by_z_on_coset
        Fr cs[2] = {ninv, zinv};
        ZK_TRY(consts.upload(cs, 2));
        w_inv = winv;
        n_inv = ninv;
        z_inv = zinv;
        ZK_TRY(pow_table(tw_fwd, w, Fr::one(), 0, 0, n / 2));
        ZK_TRY(pow_table(tw_inv, winv, Fr::one(), 0, 0, n / 2));
        // after the first inverse transform: * g^i / n, and lift the (plain or Montgomery) input
        // into Montgomery form in the same multiplication
        ZK_TRY(pow_table(s1_plain, g, ninv * r_elem, 1, 0, n));
        ZK_TRY(pow_table(s1_mont, g, ninv, 1, 0, n));
        // after the last inverse transform: * g^-i / n and drop the Montgomery factor
        ZK_TRY(pow_table(s2, ginv, ninv, 1, 1, n));
        // after the inverse transform of a or b over the derived bases: * t / n, coefficient t of x a'(x) (prove_chunk)
        ZK_TRY(pow_table(dt, Fr::one(), ninv, 3, 0, n));
        // c's inverse transform: * 1 / (n (g^n - 1)), result plain (from a plain or a Montgomery input)
        ZK_TRY(pow_table(sc_plain, Fr::one(), ninv * zinv, 2, 0, n));
        ZK_TRY(pow_table(sc_mont, Fr::one(), ninv * zinv, 2, 1, n));
        ZK_TRY(pow_table(coset_fwd, g, Fr::one(), 0, 0, n));
        ZK_TRY(pow_table(coset_inv, ginv, ninv, 2, 0, n));
        return ZK_OK;
    }

    // Run one chain of passes, in the tile form `form` (ntt_plan.h), over `batch` polynomials laid out with `stride` elements.
    // [first, first + count) cuts the launches out of the chain's pass list (the test hooks run one pass on a state of their
    // own); pre, src and bad go with the chain's first pass, post and sub with its last.
    zk_status chain(NttForm form, uint32_t* data, uint32_t batch, uint32_t stride, bool dif, bool inverse,
                    const uint32_t* pre, const uint32_t* post, const uint32_t* src = nullptr,
                    uint32_t src_stride = 0, uint32_t src_valid = 0, uint32_t* bad = nullptr,
                    const uint32_t* sub = nullptr, uint32_t sub_stride = 0, size_t first = 0, size_t count = SIZE_MAX) {
        std::vector<NttLaunch> ps;
        if (!ntt_passes(log_n, dif, stride, form, &ps)) return fail(ZK_ERR_INVALID_ARGUMENT, "no such tile form for this size");
        const uint32_t* tw = inverse ? tw_inv.as<uint32_t>() : tw_fwd.as<uint32_t>();
        for (size_t i = first; i < ps.size() && i - first < count; i++) {
            NttPass p = ps[i].pass;
            const uint32_t* s = nullptr;
            if (i == 0 && src) {
                s = src;
                p.src_stride = src_stride;
                p.src_valid = src_valid;
            }
            dim3 grid(ps[i].grid_x, batch);
            size_t shmem = ps[i].lds_bytes;
            ProfScope ps_(dif ? "ntt_pass_dif" : "ntt_pass_dit");
#ifndef ZK_EMU
            if (shmem > 65536) {
                // more than 64 KiB of dynamic LDS has to be asked for, once per device
                static std::mutex mu;
                static uint64_t raised = 0;
                std::lock_guard<std::mutex> lock(mu);
                const uint64_t bit = 1ull << (g_device & 63);
                if (!(raised & bit)) {
                    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(zkdev::k_ntt_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NTT_LDS_MAX));
                    raised |= bit;
                }
            }
#endif
            ZK_LAUNCH_SYNC(zkdev::k_ntt_pass, grid, dim3(ps[i].threads), shmem, g_stream, data, s, tw,
                           i == 0 ? pre : (const uint32_t*)nullptr,
                           i + 1 == ps.size() ? post : (const uint32_t*)nullptr, p, i == 0 && s ? bad : (uint32_t*)nullptr,
                           i + 1 == ps.size() ? sub : (const uint32_t*)nullptr, sub_stride);
        }
        if (ps.empty() && (pre || post || src)) return fail(ZK_ERR_INVALID_ARGUMENT, "size-1 transform");
        HIP_TRY(hipGetLastError());
        return ZK_OK;
    }
};

// (the MSM group - tables of a set of bases + the bucket pipeline over a list of jobs - lives in msm_group.h; its two
// instantiations are compiled in msm_g1.cpp and msm_g2.cpp, side by side with this unit)


// ------------------------------------------------------------------------------------------
// byte reader for the Parameters format
// ------------------------------------------------------------------------------------------
struct Reader {
    const uint8_t* p;
    size_t left;
    bool take(size_t n, const uint8_t** out) {
        if (left < n) return false;
        *out = p;
        p += n;
        left -= n;
        return true;
    }
    bool u32be(uint32_t* v) {
        const uint8_t* b;
        if (!take(4, &b)) return false;
        *v = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        return true;
    }
};

// bellman: the query vectors and vk.ic reject the point at infinity in both modes (Parameters::read,
// VerifyingKey::read); alpha, beta, gamma, delta are read with a plain into_affine(), which accepts it
// (in-tree twin: core/bellman-verifier/src/lib.rs:310-327) - create_proof then answers a delta at
// infinity with SynthesisError::UnexpectedIdentity.
zk_status read_g1(Reader& r, HG1A* out, const char* what, bool allow_inf = false) {
    const uint8_t* b;
    if (!r.take(96, &b)) return fail(ZK_ERR_IO, std::string("unexpected end of parameters in ") + what);
    if (zkhost::g1_from_uncompressed(b, out) != zkhost::DEC_OK) return fail(ZK_ERR_IO, std::string("invalid G1 encoding in ") + what);
    if (!allow_inf && out->is_inf()) return fail(ZK_ERR_IO, std::string("point at infinity in ") + what);
    return ZK_OK;
}
zk_status read_g2(Reader& r, HG2A* out, const char* what, bool allow_inf = false) {
    const uint8_t* b;
    if (!r.take(192, &b)) return fail(ZK_ERR_IO, std::string("unexpected end of parameters in ") + what);
    if (zkhost::g2_from_uncompressed(b, out) != zkhost::DEC_OK) return fail(ZK_ERR_IO, std::string("invalid G2 encoding in ") + what);
    if (!allow_inf && out->is_inf()) return fail(ZK_ERR_IO, std::string("point at infinity in ") + what);
    return ZK_OK;
}

bool scalar_lt_r(const uint64_t v[4]) { return !Fr::geq_p(v); }

}  // namespace

// ------------------------------------------------------------------------------------------
// zk_params
// ------------------------------------------------------------------------------------------
using zkpairs::Query;
using zkpairs::QA;
using zkpairs::QB2;
using zkpairs::QL;
using zkpairs::QB1;
// The sections the value pairs add to the two bound tables, in the order they lie there - G1: [set | pairs l | pairs b_g1 |
// pairs a | runs l | runs b_g1 | runs a | a | alpha_1 | delta_1 | b_g1 | beta_1] (the order of the C job's pair slots, prove_plan.h
// CJobLayout; the runs behind every pair section, so that the pair sections stay where a set without runs has them), G2: [b_g2 |
// beta_2 | delta_2 | pairs | runs].  ensure_derived appends by these lists and ensure_maps maps by them.
constexpr Query BOUND_G1_ORDER[3] = {QL, QB1, QA};
constexpr Query BOUND_G2_ORDER[1] = {QB2};

struct zk_params {
    // ---- what the parameter file says: plain data, a lane copies it
    struct Key {
        int device = 0;
        uint32_t n_ic = 0, n_h = 0, n_l = 0, n_a = 0, n_b1 = 0, n_b2 = 0;
        uint32_t log_m = 0;
        size_t m = 0;
        // offsets of each query inside the G1 group table (window slice 0)
        uint32_t off_h = 0, off_l = 0, off_a = 0, off_b1 = 0;
        // vk points bellman accepts at infinity (VerifyingKey::read does not reject them)
        bool alpha_g1_inf = false, beta_g1_inf = false, beta_g2_inf = false, delta_g1_inf = false, delta_g2_inf = false;
        std::vector<uint8_t> vk_bytes;   // VerifyingKey::write of the key (the head of the parameter file)
        // Entries of a query whose affine points are EQUAL (variables with identical QAP columns), found once at load from the
        // encodings: z_i P + z_j P = (z_i + z_j) P, so a job carries ONE term per distinct base and k_build_scalars sums the
        // members' scalars.  CSR, group -> member positions in the query, groups in the order of their first members; a point
        // that occurs once is in no group.  Each query on its own points: b_g1 and b_g2 need not agree.
        struct Groups {
            std::vector<uint32_t> ptr, mem;
            uint32_t count() const { return ptr.empty() ? 0u : (uint32_t)ptr.size() - 1; }
            uint32_t merged() const { return (uint32_t)mem.size() - count(); }   // entries - distinct points
        } grp_a, grp_b1, grp_b2;
    } key;
    typedef Key::Groups Groups;
    // the encodings of the three queries (the sums of two bases are made from them when the key is bound: ensure_derived, which
    // runs on the handle that loaded the key - a lane has none)
    std::vector<uint8_t> enc_a, enc_b1, enc_b2;

    // ---- the tables resident on the GPU: a lane borrows them and brings the workspaces of its own launch sets
    struct Tables {
        MsmG1 g1;
        // The two G1 jobs of a proof differ fourfold in size (A: ~15.6 k terms, C' = H + L + r B1: ~65 k for the transfer
        // circuit), so a batch runs them as TWO launch sets over the same doubling table, each with the recoding width of its
        // own size (one width for both held the large job at c = 15).  g1 = the C' set; g1a = the A set;
        // g1_lone = both jobs in one set under the width of their average, for a few proofs made alone (fewer launches).
        MsmG1 g1a, g1_lone;
        MsmG2 g2;
        // the G2 group again over the SAME table with a narrower recoding, for a proof made alone: its side stream is the
        // critical path and the depth of the bucket reduction (bit planes, doublings) is what it waits for - 256 buckets
        // instead of 2048 (c = 10 against the throughput optimum 13) cut a lone proof from 3.54 to 3.16 ms
        MsmG2 g2_lone;
        NttPlan ntt;
        // (alias(o, o.c) gives a group the c, maxd, nb and n_points of o - set_geometry with the table - and o's table borrowed)
        void share(const Tables& o) {
            g1.alias(o.g1, o.g1.c);
            g1a.alias(o.g1, o.g1a.c);
            g1_lone.alias(o.g1, o.g1_lone.c);
            g2.alias(o.g2, o.g2.c);
            g2_lone.alias(o.g2, o.g2_lone.c);
            ntt.share(o.ntt);
        }
    } tab;

    // ---- what ensure_derived binds for one (key, circuit) pair: a lane shares it
    struct Binding {
        // The derived bases of this key and ONE circuit (ensure_derived): the H query on the Lagrange basis of the domain for the
        // circuit's live rows, with the part of H that is linear in the row products folded into the bases of the variables and
        // of the rows' residuals.  g1d = [Lambda (n_rows) | E (n_rows) | D (inputs, aux) | (the value pairs' bases: prs below) | a | alpha_1 |
        // delta_1 | b_g1 | beta_1] with its own table of doublings; g1d_lone = the same table under the width of a few proofs made alone.
        struct Derived {
            bool ready = false;
            uint64_t circuit = 0;       // zk_r1cs::System::id it was built for
            uint32_t serial = 0;        // changes with every build: part of the key of the cached maps
            uint32_t n_rows = 0;        // live rows of the circuit: constraints + inputs
            uint32_t off_a = 0, off_b1 = 0;
            std::vector<int32_t> pos;   // [Lambda | E | D]: position in slice 0, or -1 for a base that came out as the identity
            double bind_ms = 0;
            bool multiples_tried = false;   // the tables were asked for their multiples once (prover_binding.h add_table_multiples)
        } drv;
        MsmG1 g1d, g1d_lone;
        // Value pairs of the (key, circuit) pair the derived set was built for (value_pairs.h; prover_binding.h derived_pairs): one
        // more base P_j + P_pred[j] per link of the circuit's chains and query that has both ends, behind the derived set in g1d (L,
        // B1 and A queries) and behind the B2 query in a table of its own, g2p.  links = [chains of A, B, L | qa | qb2 | ql | qb1] as
        // k_build_scalars reads it.  Per query (value_pairs.h Query): n = its pair bases; base = where they lie (absolute in g1d; in
        // g2p); expect = the terms a proof is expected to merge (the mean over the probe statements), for the recoding widths.
        // Value runs (value_pairs.h RUN_MAX): for every link j and l = 3 ... RUN_MAX one more base, the sum of the l chain
        // members that end at j, where the l - 1 links behind it all have their pair bases and the sum is not the identity.
        // alt[pair slot * (RUN_MAX - 2) + (l - 3)] = the base's place among the query's longer bases or -1; xbase = where those
        // lie (behind the pair sections of g1d; behind the pairs of g2p); xn = how many there are per l.  links carries one more
        // word per variable, their bits (ntt.h k_build_scalars).
        struct Pairs {
            bool ready = false;
            std::vector<int32_t> links;
            struct PerQuery {
                uint32_t n = 0, expect = 0, base = 0, xbase = 0;
                uint32_t xn[7] = {};
                std::vector<int32_t> alt;
            } q[zkpairs::N_QUERIES];
            PairCounts counts() const {
                const uint32_t n[zkpairs::N_QUERIES] = {q[QA].n, q[QB2].n, q[QL].n, q[QB1].n};
                return PairCounts::of(n);
            }
#ifdef ZK_TEST_HOOKS
            // (zk_hook_value_runs: what ensure_derived put into the tables at the places the longer bases have - G1 [l | b_g1 | a] from
            // q[QL].xbase on, G2 from q[QB2].xbase on - and the D block of the derived set, whose aux points the sums of the l query are over)
            std::vector<HG1A> hook_g1, hook_d;
            std::vector<HG2A> hook_g2;
#endif
        } prs;
        MsmG1 g1da;                     // the A jobs of a split chunk over g1d's table (its copy of the A query + the pairs)
        MsmG2 g2p, g2p_lone;            // [b_g2 | beta_2 | delta_2 | pairs | longer runs]
        // the host-side description copied, the three tables aliased under the widths o runs them at; nothing where o has none
        void share(const Binding& o) {
            if (!o.drv.ready) return;
            drv = o.drv;
            g1d.alias(o.g1d, o.g1d.c);
            g1d_lone.alias(o.g1d, o.g1d_lone.c);
            if (!o.prs.ready) return;
            prs = o.prs;
            g1da.alias(o.g1d, o.g1da.c);
            g2p.alias(o.g2p, o.g2p.c);
            g2p_lone.alias(o.g2p, o.g2p_lone.c);
        }
    } bind;

    // ---- the cache of ensure_maps for one density pattern (and one binding): every handle builds its own
    struct Maps {
        std::vector<uint8_t> dens_key;         // what the maps below were built for
        DevBuf map_a, map_b2, map_c, map_cf;   // (map_cf: the C job with the fold s * A inside, for a few proofs made alone)
        uint32_t map_nv = 0;
        DevBuf map_cd, map_cfd;         // map_c / map_cf over the derived bases
        DevBuf map_ad, map_b2d, pairs_dev;
        DevBuf alt_c, alt_a, alt_b2;    // MsmSelRange::alt of the C, A and B2 jobs: absolute table positions per pair slot and length
        PairCounts mpairs;              // the pairs the maps in use were built with (none under ZKAMD_MERGE_VALUES=0)
        // what the maps in use were built with (all 0 under ZKAMD_MERGE_BASES=0): the groups of the A, B2 and B1
        // jobs and their CSR lists in VARIABLE indices, [ptr (ga + gb2 + gb1 + 1) | members], for k_build_scalars
        uint32_t mg_a = 0, mg_b2 = 0, mg_b1 = 0;
        DevBuf grp_dev;
    } maps;

    // ---- the workspaces of a chunk: every handle has its own
    struct Work {
        DevBuf abc, wit, cvec, tail, stage_a, stage_b, stage_c, stage_w, fold_tbl, fold_c, fold_a1, fold_c1, fold_b2;
        DevBuf sel_w, sel_c;            // MsmSelRange::sel: the bytes k_build_scalars writes beside the pair slots, per proof
        PinBuf pin_g1, pin_g2, pin_tail;   // affine A, C / B of a chunk; [1 | r | s] per proof
        // [0]: raised by the kernels of a chunk that read caller scalars (non-canonical value, ONE != 1);
        // [1]: the same for the conversion pass of zk_prove_batch_witness
        DevBuf bad;
        PinBuf pin_bad;
        std::vector<MsmJob> jobs1, jobs1a, jobs2;
        std::vector<HG1> res1, res1a;
        std::vector<HG2> res2;
    } work;
};

namespace {

zk_status calibrate_kernel_forms(zk_params* P);

// The groups of equal points of one query, from its uncompressed encodings (canonical: equal bytes are equal points, and an
// encoding the decoder later refuses fails the load).  The point at infinity joins no group (in a query it fails the load as well).
void group_equal_points(const uint8_t* enc, uint32_t n, size_t size, zk_params::Groups& G) {
    std::vector<uint32_t> order;
    order.reserve(n);
    for (uint32_t i = 0; i < n; i++)
        if (!(enc[i * size] & 0x40)) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const int c = memcmp(enc + x * size, enc + y * size, size);
        return c ? c < 0 : x < y;
    });
    std::vector<std::pair<uint32_t, uint32_t>> runs;   // (first member, its place in `order`)
    for (size_t i = 0, j; i < order.size(); i = j) {
        for (j = i + 1; j < order.size() && !memcmp(enc + order[i] * size, enc + order[j] * size, size);) j++;
        if (j - i > 1) runs.push_back({order[i], (uint32_t)i});
    }
    std::sort(runs.begin(), runs.end());
    G.ptr.assign(1, 0u);
    G.mem.clear();
    for (const auto& run : runs) {
        for (size_t j = run.second; j < order.size() && !memcmp(enc + run.first * size, enc + order[j] * size, size); j++)
            G.mem.push_back(order[j]);
        G.ptr.push_back((uint32_t)G.mem.size());
    }
}

zk_status params_load(const uint8_t* pk, size_t len, int checked, int device, zk_params** out) {
    ZK_TRY(use_device(device));
    zk_params* P = new (std::nothrow) zk_params();
    if (!P) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    struct Guard {
        zk_params* p;
        ~Guard() { delete p; }
    } guard{P};
    P->key.device = device;
    Reader r{pk, len};
    HG1A alpha_g1, beta_g1, delta_g1;
    HG2A beta_g2, gamma_g2, delta_g2;
    ZK_TRY(read_g1(r, &alpha_g1, "vk.alpha_g1", true));
    ZK_TRY(read_g1(r, &beta_g1, "vk.beta_g1", true));
    ZK_TRY(read_g2(r, &beta_g2, "vk.beta_g2", true));
    ZK_TRY(read_g2(r, &gamma_g2, "vk.gamma_g2", true));
    ZK_TRY(read_g1(r, &delta_g1, "vk.delta_g1", true));
    ZK_TRY(read_g2(r, &delta_g2, "vk.delta_g2", true));
    P->key.alpha_g1_inf = alpha_g1.is_inf();
    P->key.beta_g1_inf = beta_g1.is_inf();
    P->key.beta_g2_inf = beta_g2.is_inf();
    P->key.delta_g1_inf = delta_g1.is_inf();
    P->key.delta_g2_inf = delta_g2.is_inf();
    if (!r.u32be(&P->key.n_ic)) return fail(ZK_ERR_IO, "unexpected end of parameters (ic length)");
    if ((size_t)P->key.n_ic * 96 > r.left) return fail(ZK_ERR_IO, "unexpected end of parameters in vk.ic");   // (before the allocation)
    std::vector<HG1A> ic(P->key.n_ic);
    for (uint32_t i = 0; i < P->key.n_ic; i++) ZK_TRY(read_g1(r, &ic[i], "vk.ic"));

    P->key.vk_bytes.assign(pk, pk + (len - r.left));
    // The query vectors are only LOCATED here; their 10 MB of encodings are gathered in table order and decoded on the
    // device (msm_point_kernels.h k_decode_uncompressed: round 5 - the host loop it replaces was a quarter of the load).
    // G1 table order: h | l | a | alpha_g1 | delta_g1 | b_g1 | beta_g1   (the tails carry the scalars 1, r / 1)
    // G2 table order: b_g2 | beta_g2 | delta_g2                            (scalars 1, s)
    struct Section {
        const uint8_t* at;
        uint32_t n;
        const char* what;
        bool inf_ok;   // alpha, beta, delta may be the point at infinity (bellman reads them with a plain into_affine())
    };
    auto locate = [&](uint32_t* n, size_t size, const char* what, const uint8_t** at) -> zk_status {
        if (!r.u32be(n)) return fail(ZK_ERR_IO, std::string("unexpected end of parameters (length of ") + what + ")");
        if ((size_t)*n * size > r.left) return fail(ZK_ERR_IO, std::string("unexpected end of parameters in ") + what);
        (void)r.take((size_t)*n * size, at);
        return ZK_OK;
    };
    const uint8_t *at_h, *at_l, *at_a, *at_b1, *at_b2;
    ZK_TRY(locate(&P->key.n_h, 96, "h", &at_h));
    ZK_TRY(locate(&P->key.n_l, 96, "l", &at_l));
    ZK_TRY(locate(&P->key.n_a, 96, "a", &at_a));
    ZK_TRY(locate(&P->key.n_b1, 96, "b_g1", &at_b1));
    ZK_TRY(locate(&P->key.n_b2, 192, "b_g2", &at_b2));
    group_equal_points(at_a, P->key.n_a, 96, P->key.grp_a);
    group_equal_points(at_b1, P->key.n_b1, 96, P->key.grp_b1);
    group_equal_points(at_b2, P->key.n_b2, 192, P->key.grp_b2);
    // (kept for the keys that can have value pairs alone - those of the two built-in circuits, by their counts: 6 MB for the
    //  transfer key; the points the pairs need are decoded from them a second time, on the host, when the key is bound)
    if ((P->key.n_ic == ZK_TRANSFER_N_INPUTS && P->key.n_l == ZK_TRANSFER_N_AUX) || (P->key.n_ic == ZK_ANONYMOUS_N_INPUTS && P->key.n_l == ZK_ANONYMOUS_N_AUX)) {
        P->enc_a.assign(at_a, at_a + (size_t)P->key.n_a * 96);
        P->enc_b1.assign(at_b1, at_b1 + (size_t)P->key.n_b1 * 96);
        P->enc_b2.assign(at_b2, at_b2 + (size_t)P->key.n_b2 * 192);
    }
    const Section sec1[7] = {{at_h, P->key.n_h, "h", false},       {at_l, P->key.n_l, "l", false},          {at_a, P->key.n_a, "a", false},
                             {pk, 1, "vk.alpha_g1", true},     {pk + 576, 1, "vk.delta_g1", true},  {at_b1, P->key.n_b1, "b_g1", false},
                             {pk + 96, 1, "vk.beta_g1", true}};
    const Section sec2[3] = {{at_b2, P->key.n_b2, "b_g2", false}, {pk + 192, 1, "vk.beta_g2", true}, {pk + 672, 1, "vk.delta_g2", true}};
    P->key.off_h = 0;
    P->key.off_l = P->key.n_h;
    P->key.off_a = P->key.off_l + P->key.n_l;
    P->key.off_b1 = P->key.off_a + P->key.n_a + 2;
    auto gather = [](const Section* sec, int k, size_t size, std::vector<uint8_t>& out) {
        size_t total = 0;
        for (int i = 0; i < k; i++) total += sec[i].n;
        out.resize(total * size);
        size_t at = 0;
        for (int i = 0; i < k; i++) {
            memcpy(out.data() + at, sec[i].at, (size_t)sec[i].n * size);
            at += (size_t)sec[i].n * size;
        }
        return total;
    };
    std::vector<uint8_t> enc1, enc2;
    const size_t n1 = gather(sec1, 7, 96, enc1), n2 = gather(sec2, 3, 192, enc2);
    // a refused encoding / an unexpected point at infinity is named by the query it sits in
    auto name_of = [](const Section* sec, int k, size_t idx) -> const Section& {
        for (int i = 0; i < k; i++) {
            if (idx < sec[i].n) return sec[i];
            idx -= sec[i].n;
        }
        return sec[k - 1];
    };
    auto infinity_check = [&](const Section* sec, int k, size_t size, const std::vector<uint8_t>& enc, uint32_t n_inf) -> zk_status {
        if (!n_inf) return ZK_OK;
        size_t idx = 0;
        for (int i = 0; i < k; i++)
            for (uint32_t j = 0; j < sec[i].n; j++, idx++)
                if ((enc[idx * size] & 0x40) && !sec[i].inf_ok) return fail(ZK_ERR_IO, std::string("point at infinity in ") + sec[i].what);
        return ZK_OK;
    };

    // the evaluation domain: bellman writes h with m - 1 entries
    size_t m = (size_t)P->key.n_h + 1;
    if (m < 2 || (m & (m - 1))) return fail(ZK_ERR_IO, "h query length + 1 is not a power of two");
    P->key.m = m;
    while (((size_t)1 << P->key.log_m) < m) P->key.log_m++;
    {
        // the verifying key is validated in BOTH modes (bellman reads it with the checked into_affine())
        std::vector<HG1A> vk1 = ic;
        vk1.push_back(alpha_g1);
        vk1.push_back(beta_g1);
        vk1.push_back(delta_g1);
        ZK_TRY((check_points_host<zkhost::Fq, zkdev::Fq>(vk1, "vk (G1: ic | alpha | beta | delta)")));
        ZK_TRY((check_points_host<zkhost::Fq2, DevFq2>(std::vector<HG2A>{beta_g2, gamma_g2, delta_g2}, "vk (G2: beta | gamma | delta)")));
    }
    // two G1 jobs per proof: A, and the merged C' = H + L + r * B1 - each with the width of its own size
    // (a few proofs made alone never reach the assembly level 1 of the reduction: bucket cost of the compiled few-jobs
    //  path, group 4 - ADVICE r4; the split launch sets below: group 1 / 3)
    const uint32_t c_avg = pick_window(((size_t)P->key.n_h + P->key.n_l + P->key.n_a + P->key.n_b1) / 2, 4);
    const uint32_t c1 = pick_window((size_t)P->key.n_h + P->key.n_l + P->key.n_b1, 1);
    const uint32_t c2 = pick_window(P->key.n_b2, 2);
    {
        // both groups decoded side by side, then both tables of doublings built side by side (each is one thread per base
        // walking 254 doublings: latency, not work - 19 + 23 ms one after the other)
        DevBuf raw1, raw2, map1, map2, scratch1, scratch2;
        ZK_TRY(P->tab.g1.decode_enqueue(enc1.data(), n1, c1, true, raw1, map1, g_stream));
        ZK_TRY(P->tab.g2.decode_enqueue(enc2.data(), n2, c2, true, raw2, map2, g_stream2));
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream2));
        uint32_t inf1 = 0, inf2 = 0;
        // (a refused encoding is named by its section; any other failure of the read-back - a device error - is passed on
        //  as it is: ADVICE r5, the index used to be parsed out of the message)
        size_t bad1 = (size_t)-1, bad2 = (size_t)-1;
        zk_status d1 = P->tab.g1.decode_finish("", &inf1, &bad1);
        if (d1 != ZK_OK) return bad1 != (size_t)-1 ? fail(ZK_ERR_IO, std::string("invalid G1 encoding in ") + name_of(sec1, 7, bad1).what) : d1;
        zk_status d2 = P->tab.g2.decode_finish("", &inf2, &bad2);
        if (d2 != ZK_OK) return bad2 != (size_t)-1 ? fail(ZK_ERR_IO, std::string("invalid G2 encoding in ") + name_of(sec2, 3, bad2).what) : d2;
        ZK_TRY(infinity_check(sec1, 7, 96, enc1, inf1));
        ZK_TRY(infinity_check(sec2, 3, 192, enc2, inf2));
        if (checked) {
            ZK_TRY((check_points_dev<zkhost::Fq, zkdev::Fq>(P->tab.g1.table.as<zkdev::Affine<zkdev::Fq>>(), n1, "parameters (G1)")));
            ZK_TRY((check_points_dev<zkhost::Fq2, DevFq2>(P->tab.g2.table.as<zkdev::Affine<DevFq2>>(), n2, "parameters (G2)")));
        }
        ZK_TRY(P->tab.g1.table_enqueue(scratch1, g_stream));
        ZK_TRY(P->tab.g2.table_enqueue(scratch2, g_stream2));
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream2));
    }
    P->tab.g1a.alias(P->tab.g1, pick_window(P->key.n_a, 3));
    P->tab.g1_lone.alias(P->tab.g1, c_avg);
    P->tab.g2_lone.alias(P->tab.g2, getenv("ZKAMD_WINDOW_BITS_G2") || c2 <= 10 ? c2 : 10u);
    ZK_TRY(P->tab.ntt.init(P->key.log_m));
    ZK_TRY(calibrate_kernel_forms(P));
    guard.p = nullptr;
    *out = P;
    return ZK_OK;
}

// Load-time choice between the two forms of the scratch-using assembly kernels.  One box in seventeen of
// round 4 ran the first form of exactly these two kernels at a third of its speed in every process (204 instead of 67.6 ms,
// 11.7 instead of 4.0: profiles/r04k_*_slow_box.*) - what a low scratch-wave limit looks like - while on a healthy box the
// scratch-free form is 1-2 % slower in the overlapped step.  So: when the first key is loaded on a device, one machine-filling
// launch of each form over synthetic tasks on the key's own tables (0.4 ms each, twice), and the scratch-free form is taken
// where the first form is slower than 1.4 x it.  ZKAMD_INJECT_SCRATCH_SLOW=1 (tests) triples the first form's measured time.
zk_status calibrate_kernel_forms(zk_params* P) {
#if defined(ZK_HAVE_MADD_ASM) && defined(ZK_HAVE_RED_ASM)
    std::lock_guard<std::mutex> lock(g_forms_mu);
    KernelForms& F = g_forms[P->key.device & 63];
    if (F.done) return ZK_OK;
    const uint32_t n2 = (uint32_t)std::min<size_t>(P->tab.g2.n_points * (size_t)zkdev::MSM_NPOS, 1u << 24);
    const uint32_t n1 = (uint32_t)std::min<size_t>(P->tab.g1.n_points * (size_t)zkdev::MSM_NPOS, 1u << 24);
    if (n1 < 1024 || n2 < 1024 || getenv("ZKAMD_NO_CALIBRATE")) {   // (a toy key: nothing to measure on, the first form stays)
        F.done = true;
        return ZK_OK;
    }
    // each half next to the kernels it launches (msm_g2.cpp, msm_g1.cpp)
    ZK_TRY(calibrate_g2_accumulate(P->tab.g2.table.as<zkdev::Affine<DevFq2>>(), n2, &F.ms[0]));
    ZK_TRY(calibrate_g1_reduce(P->tab.g1.table.as<zkdev::Affine<zkdev::Fq28>>(), n1, &F.ms[2]));
    const float slow = hook_env("ZKAMD_INJECT_SCRATCH_SLOW") && atoi(hook_env("ZKAMD_INJECT_SCRATCH_SLOW")) ? 3.0f : 1.0f;
    F.ms[0] *= slow;
    F.ms[2] *= slow;
    F.form[0] = F.ms[0] > 1.4f * F.ms[1] ? 1u : 0u;
    F.form[1] = F.ms[2] > 1.4f * F.ms[3] ? 1u : 0u;
    F.done = true;
#else
    (void)P;
#endif
    return ZK_OK;
}

// A second handle over the SAME key for another lane of a pipeline: the tables (doubling tables, NTT tables)
// are borrowed, the per-chunk workspaces are its own.  The original must outlive the clone.
zk_params* params_clone_for_lane(const zk_params* P) {
    zk_params* Q = new (std::nothrow) zk_params();
    if (!Q) return nullptr;
    Q->key = P->key;
    Q->tab.share(P->tab);
    Q->bind.share(P->bind);
    return Q;
}
// ... and over the same circuit: the matrices are borrowed, the assignment and the witness generator's state are its own
zk_r1cs* r1cs_clone_for_lane(const zk_r1cs* R) {
    zk_r1cs* Q = new (std::nothrow) zk_r1cs();
    if (!Q) return nullptr;
    Q->sys.share(R->sys);
    return Q;
}

}  // namespace
