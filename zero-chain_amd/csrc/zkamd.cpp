// libzkamd: host orchestration + C ABI (include/zkamd.h) of the MI355X Groth16 prover hot path.
//
// What it replaces in the reference (all behind core/proofs/src/confidential.rs:149, in the
// un-vendored bellman 0.1.0 crate; restated in SURVEY.md Appendix A):
//   create_proof step 3  (EvaluationDomain H pipeline)   -> ntt.h kernels, NttPlan below
//   create_proof step 4  (8 x multiexp)                  -> msm.h kernels, MsmGroup below
//   create_proof step 6  (final fold, into_affine)       -> k_ct_scale_add (coop_tail.cpp) / k_xyzz_normalize_export (msm.h)
//   Parameters::read                                     -> Params::load below
//   Proof::write                                         -> host_math.h g1/g2_to_compressed
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <thread>
#include <chrono>
#include <algorithm>
#include <new>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <deque>
#if defined(__linux__)
#include <sched.h>
#endif

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

    zk_status upload_fr(DevBuf& buf, const Fr* v, size_t count) {
        ZK_TRY(buf.ensure(count * 32));
        HIP_TRY(hipMemcpy(buf.p, v, count * 32, hipMemcpyHostToDevice));
        return ZK_OK;
    }

    zk_status pow_table(DevBuf& out, const Fr& base, const Fr& scale, uint32_t mode, uint32_t raw, size_t count) {
        DevBuf tmp;
        Fr bs[2] = {base, scale};
        ZK_TRY(upload_fr(tmp, bs, 2));
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
        ZK_TRY(upload_fr(consts, cs, 2));
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
struct zk_params {
    int device = 0;
    uint32_t n_ic = 0, n_h = 0, n_l = 0, n_a = 0, n_b1 = 0, n_b2 = 0;
    uint32_t log_m = 0;
    size_t m = 0;
    // offsets of each query inside the G1 group table (window slice 0)
    uint32_t off_h = 0, off_l = 0, off_a = 0, off_b1 = 0;
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
    // The derived bases of this key and ONE circuit (ensure_derived): the H query on the Lagrange basis of the domain for the
    // circuit's live rows, with the part of H that is linear in the row products folded into the bases of the variables and
    // of the rows' residuals.  g1d = [Lambda (n_rows) | E (n_rows) | D (inputs, aux) | (the value pairs' bases: prs below) | a | alpha_1 |
    // delta_1 | b_g1 | beta_1] with its own table of doublings; g1d_lone = the same table under the width of a few proofs made alone.
    struct Derived {
        bool ready = false;
        uint64_t circuit = 0;       // zk_r1cs::id it was built for
        uint32_t serial = 0;        // changes with every build: part of the key of the cached maps
        uint32_t n_rows = 0;        // live rows of the circuit: constraints + inputs
        uint32_t off_a = 0, off_b1 = 0;
        std::vector<int32_t> pos;   // [Lambda | E | D]: position in slice 0, or -1 for a base that came out as the identity
        double bind_ms = 0;
    } drv;
    MsmG1 g1d, g1d_lone;
    DevBuf map_cd, map_cfd;         // map_c / map_cf over the derived bases
    // Value pairs of the (key, circuit) pair the derived set was built for (value_pairs.h; derived_pairs below): one more
    // base P_j + P_pred[j] per link of the circuit's chains and query that has both ends, behind the derived set in g1d (L, B1
    // and A queries) and behind the B2 query in a table of its own, g2p.  links = [chains of A, B, L | qa | qb2 | ql | qb1] as
    // k_build_scalars reads it; base_* = where the pair bases lie (absolute in g1d; in g2p); exp_* = the terms a proof is
    // expected to merge per query (the mean over the probe statements), for the recoding widths.
    struct Pairs {
        bool ready = false;
        std::vector<int32_t> links;
        uint32_t base_l = 0, base_b1 = 0, base_a = 0, base_b2 = 0;
        PairCounts n;
        uint32_t exp_a = 0, exp_b2 = 0, exp_l = 0, exp_b1 = 0;
        // Value runs (value_pairs.h RUN_MAX): for every link j and l = 3 ... RUN_MAX one more base, the sum of the l chain
        // members that end at j, where the l - 1 links behind it all have their pair bases and the sum is not the identity.
        // Per query [a | b_g2 | l | b_g1]: alt[pair slot * (RUN_MAX - 2) + (l - 3)] = the base's place among the query's
        // longer bases or -1; xbase = where those lie (behind the pair sections of g1d; behind the pairs of g2p); xn = how
        // many there are per l.  links carries one more word per variable, their bits (ntt.h k_build_scalars).
        std::vector<int32_t> alt[4];
        uint32_t xbase[4] = {0, 0, 0, 0};
        uint32_t xn[4][7] = {};
#ifdef ZK_TEST_HOOKS
        // (zk_hook_value_runs: what ensure_derived put into the tables at the places the longer bases have - G1 [l | b_g1 | a] from
        // xbase[2] on, G2 from xbase[1] on - and the D block of the derived set, whose aux points the sums of the l query are over)
        std::vector<HG1A> hook_g1, hook_d;
        std::vector<HG2A> hook_g2;
#endif
    } prs;
    MsmG1 g1da;                     // the A jobs of a split chunk over g1d's table (its copy of the A query + the pairs)
    MsmG2 g2p, g2p_lone;            // [b_g2 | beta_2 | delta_2 | pairs | longer runs]
    DevBuf map_ad, map_b2d, pairs_dev;
    DevBuf alt_c, alt_a, alt_b2;    // MsmSelRange::alt of the C, A and B2 jobs: absolute table positions per pair slot and length
    DevBuf sel_w, sel_c;            // MsmSelRange::sel: the bytes k_build_scalars writes beside the pair slots, per proof
    PairCounts mpairs;              // the pairs the maps in use were built with (ensure_maps; none under ZKAMD_MERGE_VALUES=0)
    std::vector<uint8_t> enc_a, enc_b1, enc_b2;   // the encodings of the three queries (the sums of two bases are made from them)
    // cached per-circuit index maps (keyed by the density bytes)
    std::vector<uint8_t> dens_key;
    DevBuf map_a, map_b2, map_c, map_cf;   // (map_cf: the C job with the fold s * A inside, for a few proofs made alone)
    uint32_t map_nv = 0;
    // Entries of a query whose affine points are EQUAL (variables with identical QAP columns), found once at load from the
    // encodings: z_i P + z_j P = (z_i + z_j) P, so a job carries ONE term per distinct base and k_build_scalars sums the
    // members' scalars.  CSR, group -> member positions in the query, groups in the order of their first members; a point
    // that occurs once is in no group.  Each query on its own points: b_g1 and b_g2 need not agree.
    struct Groups {
        std::vector<uint32_t> ptr, mem;
        uint32_t count() const { return ptr.empty() ? 0u : (uint32_t)ptr.size() - 1; }
        uint32_t merged() const { return (uint32_t)mem.size() - count(); }   // entries - distinct points
    } grp_a, grp_b1, grp_b2;
    // what the maps in use were built with (ensure_maps; all 0 under ZKAMD_MERGE_BASES=0): the groups of the A, B2 and B1
    // jobs and their CSR lists in VARIABLE indices, [ptr (ga + gb2 + gb1 + 1) | members], for k_build_scalars
    uint32_t mg_a = 0, mg_b2 = 0, mg_b1 = 0;
    DevBuf grp_dev;
    // workspaces
    DevBuf abc, wit, cvec, tail, stage_a, stage_b, stage_c, stage_w, fold_tbl, fold_c, fold_a1, fold_c1, fold_b2;
    PinBuf pin_g1, pin_g2, pin_tail;   // affine A, C / B of a chunk; [1 | r | s] per proof
    // [0]: raised by the kernels of a chunk that read caller scalars (non-canonical value, ONE != 1);
    // [1]: the same for the conversion pass of zk_prove_batch_witness
    DevBuf bad;
    PinBuf pin_bad;
    // vk points bellman accepts at infinity (VerifyingKey::read does not reject them)
    bool alpha_g1_inf = false, beta_g1_inf = false, beta_g2_inf = false, delta_g1_inf = false, delta_g2_inf = false;
    std::vector<uint8_t> vk_bytes;   // VerifyingKey::write of the key (the head of the parameter file)
    std::vector<MsmJob> jobs1, jobs1a, jobs2;
    std::vector<HG1> res1, res1a;
    std::vector<HG2> res2;
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
    P->device = device;
    Reader r{pk, len};
    HG1A alpha_g1, beta_g1, delta_g1;
    HG2A beta_g2, gamma_g2, delta_g2;
    ZK_TRY(read_g1(r, &alpha_g1, "vk.alpha_g1", true));
    ZK_TRY(read_g1(r, &beta_g1, "vk.beta_g1", true));
    ZK_TRY(read_g2(r, &beta_g2, "vk.beta_g2", true));
    ZK_TRY(read_g2(r, &gamma_g2, "vk.gamma_g2", true));
    ZK_TRY(read_g1(r, &delta_g1, "vk.delta_g1", true));
    ZK_TRY(read_g2(r, &delta_g2, "vk.delta_g2", true));
    P->alpha_g1_inf = alpha_g1.is_inf();
    P->beta_g1_inf = beta_g1.is_inf();
    P->beta_g2_inf = beta_g2.is_inf();
    P->delta_g1_inf = delta_g1.is_inf();
    P->delta_g2_inf = delta_g2.is_inf();
    if (!r.u32be(&P->n_ic)) return fail(ZK_ERR_IO, "unexpected end of parameters (ic length)");
    if ((size_t)P->n_ic * 96 > r.left) return fail(ZK_ERR_IO, "unexpected end of parameters in vk.ic");   // (before the allocation)
    std::vector<HG1A> ic(P->n_ic);
    for (uint32_t i = 0; i < P->n_ic; i++) ZK_TRY(read_g1(r, &ic[i], "vk.ic"));

    P->vk_bytes.assign(pk, pk + (len - r.left));
    // The query vectors are only LOCATED here; their 10 MB of encodings are gathered in table order and decoded on the
    // device (msm.h k_decode_uncompressed: round 5 - the host loop it replaces was a quarter of the load).
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
    ZK_TRY(locate(&P->n_h, 96, "h", &at_h));
    ZK_TRY(locate(&P->n_l, 96, "l", &at_l));
    ZK_TRY(locate(&P->n_a, 96, "a", &at_a));
    ZK_TRY(locate(&P->n_b1, 96, "b_g1", &at_b1));
    ZK_TRY(locate(&P->n_b2, 192, "b_g2", &at_b2));
    group_equal_points(at_a, P->n_a, 96, P->grp_a);
    group_equal_points(at_b1, P->n_b1, 96, P->grp_b1);
    group_equal_points(at_b2, P->n_b2, 192, P->grp_b2);
    // (kept for the keys that can have value pairs alone - those of the two built-in circuits, by their counts: 6 MB for the
    //  transfer key; the points the pairs need are decoded from them a second time, on the host, when the key is bound)
    if ((P->n_ic == ZK_TRANSFER_N_INPUTS && P->n_l == ZK_TRANSFER_N_AUX) || (P->n_ic == ZK_ANONYMOUS_N_INPUTS && P->n_l == ZK_ANONYMOUS_N_AUX)) {
        P->enc_a.assign(at_a, at_a + (size_t)P->n_a * 96);
        P->enc_b1.assign(at_b1, at_b1 + (size_t)P->n_b1 * 96);
        P->enc_b2.assign(at_b2, at_b2 + (size_t)P->n_b2 * 192);
    }
    const Section sec1[7] = {{at_h, P->n_h, "h", false},       {at_l, P->n_l, "l", false},          {at_a, P->n_a, "a", false},
                             {pk, 1, "vk.alpha_g1", true},     {pk + 576, 1, "vk.delta_g1", true},  {at_b1, P->n_b1, "b_g1", false},
                             {pk + 96, 1, "vk.beta_g1", true}};
    const Section sec2[3] = {{at_b2, P->n_b2, "b_g2", false}, {pk + 192, 1, "vk.beta_g2", true}, {pk + 672, 1, "vk.delta_g2", true}};
    P->off_h = 0;
    P->off_l = P->n_h;
    P->off_a = P->off_l + P->n_l;
    P->off_b1 = P->off_a + P->n_a + 2;
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
    size_t m = (size_t)P->n_h + 1;
    if (m < 2 || (m & (m - 1))) return fail(ZK_ERR_IO, "h query length + 1 is not a power of two");
    P->m = m;
    while (((size_t)1 << P->log_m) < m) P->log_m++;
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
    const uint32_t c_avg = pick_window(((size_t)P->n_h + P->n_l + P->n_a + P->n_b1) / 2, 4);
    const uint32_t c1 = pick_window((size_t)P->n_h + P->n_l + P->n_b1, 1);
    const uint32_t c2 = pick_window(P->n_b2, 2);
    {
        // both groups decoded side by side, then both tables of doublings built side by side (each is one thread per base
        // walking 254 doublings: latency, not work - 19 + 23 ms one after the other)
        DevBuf raw1, raw2, map1, map2, scratch1, scratch2;
        ZK_TRY(P->g1.decode_enqueue(enc1.data(), n1, c1, true, raw1, map1, g_stream));
        ZK_TRY(P->g2.decode_enqueue(enc2.data(), n2, c2, true, raw2, map2, g_stream2));
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream2));
        uint32_t inf1 = 0, inf2 = 0;
        // (a refused encoding is named by its section; any other failure of the read-back - a device error - is passed on
        //  as it is: ADVICE r5, the index used to be parsed out of the message)
        size_t bad1 = (size_t)-1, bad2 = (size_t)-1;
        zk_status d1 = P->g1.decode_finish("", &inf1, &bad1);
        if (d1 != ZK_OK) return bad1 != (size_t)-1 ? fail(ZK_ERR_IO, std::string("invalid G1 encoding in ") + name_of(sec1, 7, bad1).what) : d1;
        zk_status d2 = P->g2.decode_finish("", &inf2, &bad2);
        if (d2 != ZK_OK) return bad2 != (size_t)-1 ? fail(ZK_ERR_IO, std::string("invalid G2 encoding in ") + name_of(sec2, 3, bad2).what) : d2;
        ZK_TRY(infinity_check(sec1, 7, 96, enc1, inf1));
        ZK_TRY(infinity_check(sec2, 3, 192, enc2, inf2));
        if (checked) {
            ZK_TRY((check_points_dev<zkhost::Fq, zkdev::Fq>(P->g1.table.as<zkdev::Affine<zkdev::Fq>>(), n1, "parameters (G1)")));
            ZK_TRY((check_points_dev<zkhost::Fq2, DevFq2>(P->g2.table.as<zkdev::Affine<DevFq2>>(), n2, "parameters (G2)")));
        }
        ZK_TRY(P->g1.table_enqueue(scratch1, g_stream));
        ZK_TRY(P->g2.table_enqueue(scratch2, g_stream2));
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream2));
    }
    P->g1a.alias(P->g1, pick_window(P->n_a, 3));
    P->g1_lone.alias(P->g1, c_avg);
    P->g2_lone.alias(P->g2, getenv("ZKAMD_WINDOW_BITS_G2") || c2 <= 10 ? c2 : 10u);
    ZK_TRY(P->ntt.init(P->log_m));
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
    KernelForms& F = g_forms[P->device & 63];
    if (F.done) return ZK_OK;
    const uint32_t n2 = (uint32_t)std::min<size_t>(P->g2.n_points * (size_t)zkdev::MSM_NPOS, 1u << 24);
    const uint32_t n1 = (uint32_t)std::min<size_t>(P->g1.n_points * (size_t)zkdev::MSM_NPOS, 1u << 24);
    if (n1 < 1024 || n2 < 1024 || getenv("ZKAMD_NO_CALIBRATE")) {   // (a toy key: nothing to measure on, the first form stays)
        F.done = true;
        return ZK_OK;
    }
    // each half next to the kernels it launches (msm_g2.cpp, msm_g1.cpp)
    ZK_TRY(calibrate_g2_accumulate(P->g2.table.as<zkdev::Affine<DevFq2>>(), n2, &F.ms[0]));
    ZK_TRY(calibrate_g1_reduce(P->g1.table.as<zkdev::Affine<zkdev::Fq28>>(), n1, &F.ms[2]));
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
    Q->device = P->device;
    Q->n_ic = P->n_ic; Q->n_h = P->n_h; Q->n_l = P->n_l; Q->n_a = P->n_a; Q->n_b1 = P->n_b1; Q->n_b2 = P->n_b2;
    Q->log_m = P->log_m;
    Q->m = P->m;
    Q->off_h = P->off_h; Q->off_l = P->off_l; Q->off_a = P->off_a; Q->off_b1 = P->off_b1;
    Q->g1.alias(P->g1, P->g1.c);
    Q->g1a.alias(P->g1, P->g1a.c);
    Q->g1_lone.alias(P->g1, P->g1_lone.c);
    Q->g2.c = P->g2.c; Q->g2.maxd = P->g2.maxd; Q->g2.nb = P->g2.nb; Q->g2.n_points = P->g2.n_points;
    Q->g2.table.borrow(P->g2.table);
    Q->g2_lone.alias(P->g2, P->g2_lone.c);
    if (P->drv.ready) {
        Q->drv = P->drv;
        Q->g1d.alias(P->g1d, P->g1d.c);
        Q->g1d_lone.alias(P->g1d, P->g1d_lone.c);
        if (P->prs.ready) {
            Q->prs = P->prs;
            Q->g1da.alias(P->g1d, P->g1da.c);
            Q->g2p.c = P->g2p.c; Q->g2p.maxd = P->g2p.maxd; Q->g2p.nb = P->g2p.nb; Q->g2p.n_points = P->g2p.n_points;
            Q->g2p.table.borrow(P->g2p.table);
            Q->g2p_lone.alias(P->g2p, P->g2p_lone.c);
        }
    }
    Q->ntt.log_n = P->ntt.log_n;
    Q->ntt.n = P->ntt.n;
    Q->ntt.tw_fwd.borrow(P->ntt.tw_fwd);
    Q->ntt.tw_inv.borrow(P->ntt.tw_inv);
    Q->ntt.s1_plain.borrow(P->ntt.s1_plain);
    Q->ntt.s1_mont.borrow(P->ntt.s1_mont);
    Q->ntt.s2.borrow(P->ntt.s2);
    Q->ntt.dt.borrow(P->ntt.dt);
    Q->ntt.sc_plain.borrow(P->ntt.sc_plain);
    Q->ntt.sc_mont.borrow(P->ntt.sc_mont);
    Q->ntt.coset_fwd.borrow(P->ntt.coset_fwd);
    Q->ntt.coset_inv.borrow(P->ntt.coset_inv);
    Q->ntt.consts.borrow(P->ntt.consts);
    Q->alpha_g1_inf = P->alpha_g1_inf; Q->beta_g1_inf = P->beta_g1_inf; Q->beta_g2_inf = P->beta_g2_inf;
    Q->delta_g1_inf = P->delta_g1_inf; Q->delta_g2_inf = P->delta_g2_inf;
    Q->vk_bytes = P->vk_bytes;
    Q->grp_a = P->grp_a; Q->grp_b1 = P->grp_b1; Q->grp_b2 = P->grp_b2;
    return Q;
}
zk_r1cs* r1cs_clone_for_lane(const zk_r1cs* R) {
    zk_r1cs* Q = new (std::nothrow) zk_r1cs();
    if (!Q) return nullptr;
    Q->device = R->device;
    Q->id = R->id;
    Q->n_in = R->n_in; Q->n_aux = R->n_aux; Q->n_con = R->n_con;
    for (int m = 0; m < 3; m++) {
        Q->row_ptr[m].borrow(R->row_ptr[m]);
        Q->col[m].borrow(R->col[m]);
        Q->coeff[m].borrow(R->coeff[m]);
    }
    Q->a_aux_density = R->a_aux_density;
    Q->b_input_density = R->b_input_density;
    Q->b_aux_density = R->b_aux_density;
    return Q;
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
    for (int i = 0; i < 4; i++) key.push_back((uint8_t)((P->drv.ready ? P->drv.serial : 0u) >> (8 * i)));
    key.push_back(merge ? 1 : 0);
    const uint32_t nv = n_in + n_aux;
    // value pairs: over the derived set that carries them (its serial is in the key), unless ZKAMD_MERGE_VALUES=0
    const bool pairs = merge_values_on() && P->drv.ready && P->prs.ready && P->prs.links.size() == 11 * (size_t)nv;
    key.push_back(pairs ? 1 : 0);
    if (key == P->dens_key) return ZK_OK;
    const PairCounts pc = pairs ? P->prs.n : PairCounts();
    // scalar layout per proof: [inputs | aux | 1 | r | s | sums of the A groups | sums of the B2 groups] (prove_plan.h CJobLayout)
    std::vector<int32_t> ma(nv + 3, -1), mb1(nv + 3, -1), mb2(nv + 3, -1);
    std::vector<uint32_t> var_a, var_b;   // query position -> variable
    var_a.reserve(P->n_a);
    var_b.reserve(P->n_b1);
    uint32_t pa = n_in;
    for (uint32_t i = 0; i < n_in; i++) {   // A inputs: full density
        ma[i] = (int32_t)i;
        var_a.push_back(i);
    }
    for (uint32_t j = 0; j < n_aux; j++)
        if (a_aux_d[j]) {
            ma[n_in + j] = (int32_t)pa++;
            var_a.push_back(n_in + j);
        }
    // bellman's generator emits exactly one `a` entry per input and per dense aux variable (and the
    // b queries likewise): a different count means the assignment belongs to another circuit than the key
    if (pa != P->n_a)
        return fail(ZK_ERR_IO, "the A density of the assignment (" + std::to_string(pa) + ") differs from the key's a query (" +
                                   std::to_string(P->n_a) + ")");
    if (!P->alpha_g1_inf) ma[nv] = (int32_t)P->n_a;   // 1 * alpha_g1
    ma[nv + 1] = (int32_t)P->n_a + 1;                 // r * delta_g1 (never at infinity here: prove_* refuse)
    uint32_t pb = 0;
    for (uint32_t i = 0; i < n_in; i++)
        if (b_in_d[i]) {
            mb1[i] = mb2[i] = (int32_t)pb++;
            var_b.push_back(i);
        }
    for (uint32_t j = 0; j < n_aux; j++)
        if (b_aux_d[j]) {
            mb1[n_in + j] = mb2[n_in + j] = (int32_t)pb++;
            var_b.push_back(n_in + j);
        }
    if (pb != P->n_b1 || pb != P->n_b2)
        return fail(ZK_ERR_IO, "the B density of the assignment (" + std::to_string(pb) + ") differs from the key's b queries (" +
                                   std::to_string(P->n_b1) + " in G1, " + std::to_string(P->n_b2) + " in G2)");
    if (!P->beta_g1_inf) mb1[nv] = (int32_t)P->n_b1;   // 1 * beta_g1
    if (!P->beta_g2_inf) mb2[nv] = (int32_t)P->n_b2;   // 1 * beta_g2
    mb2[nv + 2] = (int32_t)P->n_b2 + 1;                // s * delta_g2
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
    mute(merge ? P->grp_a : none, var_a, ma, base_a);
    mute(merge ? P->grp_b2 : none, var_b, mb2, base_b2);
    mute(merge ? P->grp_b1 : none, var_b, mb1, base_b1);
    const uint32_t ga = (uint32_t)base_a.size(), gb2 = (uint32_t)base_b2.size(), gb1 = (uint32_t)base_b1.size();
    // (each of the two jobs over this vector selects its own sums; the other's stay -1)
    const CJobLayout W = cjob_layout(n_in, n_aux, (uint32_t)P->m, ga, gb2, gb1, false, false);
    ma.resize(W.wstride, -1);
    mb2.resize(W.wstride, -1);
    for (uint32_t g = 0; g < ga; g++) ma[W.w_sum_a + g] = base_a[g];
    for (uint32_t g = 0; g < gb2; g++) mb2[W.w_sum_b2 + g] = base_b2[g];
    // h coefficients leave the last transform in bit-reversed order; the top coefficient
    // (degree m - 1) is dropped exactly as bellman truncates it
    std::vector<int32_t> mh(P->m);
    for (size_t pos = 0; pos < P->m; pos++) {
        uint32_t e = P->log_m ? (__builtin_bitreverse32((uint32_t)pos) >> (32 - P->log_m)) : 0;
        mh[pos] = e < P->n_h ? (int32_t)e : -1;
    }
    auto upload = [](DevBuf& dst, const auto& v) -> zk_status {
        ZK_TRY(dst.ensure(v.size() * 4));
        HIP_TRY(hipMemcpy(dst.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return ZK_OK;
    };
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
            section(L.pair_l);
            for (uint32_t k = 0; k < L.pl; k++) map.push_back((int32_t)(P->prs.base_l + k));
            section(L.pair_b1);
            for (uint32_t k = 0; k < L.pb1; k++) map.push_back((int32_t)(P->prs.base_b1 + k));
            if (L.fold) {
                section(L.pair_a);
                for (uint32_t k = 0; k < L.pa; k++) map.push_back((int32_t)(P->prs.base_a + k));
            }
        }
        section(L.cstride);
        if (!fits) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: the C map does not follow its layout");
        return upload(dst, map);
    };
    std::vector<int32_t> hk;   // the key's own bases: [h (m) | l (n_aux)]
    hk.reserve(P->m + n_aux);
    for (size_t pos = 0; pos < P->m; pos++) hk.push_back(mh[pos] < 0 ? -1 : (int32_t)(P->off_h + mh[pos]));
    for (uint32_t j = 0; j < n_aux; j++) hk.push_back((int32_t)(P->off_l + j));
    for (bool fold : {false, true})
        ZK_TRY(upload_c_map(fold ? P->map_cf : P->map_c, cjob_layout(n_in, n_aux, (uint32_t)P->m, ga, gb2, gb1, fold, false), hk.data(),
                            hk.data() + P->m, nullptr, P->off_a, P->off_b1));
    if (P->drv.ready && P->drv.pos.size() == 2 * (size_t)P->drv.n_rows + nv) {
        // the same job over the derived bases, pos = [s (n_rows) | e (n_rows) | inputs | aux]
        const zk_params::Derived& D = P->drv;
        const uint32_t head = 2 * D.n_rows;
        for (bool fold : {false, true})
            ZK_TRY(upload_c_map(fold ? P->map_cfd : P->map_cd, cjob_layout(n_in, n_aux, head, ga, gb2, gb1, fold, true, pc), D.pos.data(),
                                D.pos.data() + head + n_in, D.pos.data() + head, D.off_a, D.off_b1));
    }
    if (pairs) {
        // The A and B2 jobs of a chunk with pairs: the A map in absolute positions of the derived table (its copy of the A query,
        // the pair bases in front of it), the B2 map over its own copy of the variables' slots and the table with its pairs
        const CJobLayout Wp = cjob_layout(n_in, n_aux, 0, ga, gb2, gb1, false, true, pc);
        std::vector<int32_t> mad(Wp.wstride, -1), mbd(Wp.wstride, -1);
        for (uint32_t i = 0; i < W.wstride; i++) {
            if (ma[i] >= 0) mad[i] = (int32_t)(P->drv.off_a + ma[i]);
            if (i >= nv) mbd[i] = mb2[i];
        }
        for (uint32_t i = 0; i < nv; i++) mbd[Wp.w_b2v + i] = mb2[i];
        for (uint32_t k = 0; k < pc.a; k++) mad[Wp.w_pair_a + k] = (int32_t)(P->prs.base_a + k);
        for (uint32_t k = 0; k < pc.b2; k++) mbd[Wp.w_pair_b2 + k] = (int32_t)(P->prs.base_b2 + k);
        ZK_TRY(upload(P->map_ad, mad));
        ZK_TRY(upload(P->map_b2d, mbd));
        ZK_TRY(upload(P->pairs_dev, P->prs.links));
        // MsmSelRange::alt: per pair slot of the job, in the order of its sections, the table positions of the longer bases
        auto alts = [&](std::initializer_list<uint32_t> queries) {
            std::vector<int32_t> out;
            for (uint32_t query : queries)
                for (int32_t x : P->prs.alt[query]) out.push_back(x < 0 ? -1 : (int32_t)(P->prs.xbase[query] + (uint32_t)x));
            if (out.empty()) out.push_back(-1);
            return out;
        };
        if (zkpairs::RUN_MAX > 2) {
            ZK_TRY(upload(P->alt_c, alts({2u, 3u, 0u})));   // [pl | pb1 | (fold: pa)]
            ZK_TRY(upload(P->alt_a, alts({0u})));
            ZK_TRY(upload(P->alt_b2, alts({1u})));
        }
    }
    gptr.insert(gptr.end(), gmem.begin(), gmem.end());
    ZK_TRY(upload(P->grp_dev, gptr));
    ZK_TRY(upload(P->map_a, ma));
    ZK_TRY(upload(P->map_b2, mb2));
    P->dens_key.swap(key);
    P->map_nv = nv;
    P->mg_a = ga;
    P->mg_b2 = gb2;
    P->mg_b1 = gb1;
    P->mpairs = pc;
    return ZK_OK;
}

// create_proof step 6, rearranged:  with A = alpha + sum_A + r*delta (already
// complete, the alpha and r*delta terms rode along in the A multiexp) and
// C' = h + l + r*(beta_1 + sum_B1) from the merged multiexp,
//   C = s*A + C'   ==  rs*delta + s*alpha + r*beta_1 + s*sum_A + r*sum_B1 + h + l.
// (prove_chunk: the fold and the three into_affine run on the GPU, k_ct_scale_add /
// k_xyzz_normalize_export; the host encodes the 192 bytes.)

// One chunk of proofs: the plan (prove_plan.h), what its stages hand to each other, and the stages in the order they run.
// derived: a, b, c are the library's own row evaluations of the circuit P->drv was built for - the four-transform form over
// the derived bases (ensure_derived), whose H scalars are those of the live rows.
static_assert(zkpairs::RUN_MAX <= zkdev::PAIR_RUN_CAP, "k_build_scalars holds a block of a run in one 64-bit word");
static_assert(PROVE_FOLD_IN_MSM_MAX == MSM_FEW_JOBS, "the fold rides in the multiexp up to the few-jobs limit of a launch set");
typedef zkdev::XYZZ<zkdev::Fq> DP1;
struct ChunkRun {
    zk_params* P;
    size_t np;
    const zk_batch_dev* bt;
    size_t first;            // the chunk's first proof in the batch
    bool derived, mont;
    ProvePlan plan;
    hipStream_t side;        // the G2 set and the A jobs of a split chunk run here, beside the H pipeline
    MsmG2* G2;
    MsmG1* G1C;              // the group of the C' jobs
    const int32_t* map_c;
    uint32_t *wit, *cvec, *bad;
    const DP1* a_dev = nullptr;   // A of every proof, where the G1 launch sets left it
    bool pairs = false;      // the layout has the sections of the value pairs: the A and B2 jobs over their tables and maps
    static constexpr uint32_t RUN_W = zkpairs::RUN_MAX - 2;   // longer bases per pair slot (none: the jobs go without bytes)

    // ---- scalars [inputs | aux | 1 | r | s | sums of the A groups | of the B2 groups] per proof, plain, and the merged C job's
    // but for its H block (prove_plan.h CJobLayout)
    zk_status scalars(const uint8_t* rs) {
        const CJobLayout& L = plan.layout;
        const uint32_t nv = L.n_in + L.n_aux;
        ZK_TRY(P->wit.ensure(np * (size_t)L.wstride * 32));
        wit = P->wit.as<uint32_t>();
        ZK_TRY(P->pin_tail.ensure(np * 96));
        uint8_t* tail = P->pin_tail.as<uint8_t>();
        memset(tail, 0, np * 96);
        std::vector<uint64_t> rsv(np * 8);
        for (size_t p = 0; p < np; p++) {
            const uint8_t* rr = rs + (first + p) * 64;
            load_scalar_le(rr, &rsv[p * 8]);
            load_scalar_le(rr + 32, &rsv[p * 8 + 4]);
            if (!scalar_lt_r(&rsv[p * 8]) || !scalar_lt_r(&rsv[p * 8 + 4]))
                return fail(ZK_ERR_INVALID_ARGUMENT, "r or s is not a canonical scalar (>= field modulus)");
            tail[p * 96] = 1;
            memcpy(&tail[p * 96 + 32], rr, 64);
        }
        ZK_TRY(P->tail.ensure(np * 96));
        HIP_TRY(hipMemcpyAsync(P->tail.p, tail, np * 96, hipMemcpyHostToDevice, g_stream));
        ZK_TRY(P->bad.ensure(8));
        ZK_TRY(P->pin_bad.ensure(8));
        bad = P->bad.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(bad, 0, 4, g_stream));
        ZK_TRY(P->cvec.ensure(np * (size_t)L.cstride * 32));
        cvec = P->cvec.as<uint32_t>();
        const bool bytes = pairs && RUN_W;   // (at RUN_MAX = 2 a pair slot is its pair: nothing to name)
        if (bytes) {   // (every byte is written: by the thread that writes its pair slot)
            ZK_TRY(P->sel_w.ensure(np * (size_t)L.sel_w + 1));
            ZK_TRY(P->sel_c.ensure(np * (size_t)L.sel_c + 1));
        }
        // (the same launch: a thread per variable, three for the tail, one per group)
        ZK_LAUNCH(zkdev::k_build_scalars, dim3((L.w_end + L.gb1 + 255) / 256, (unsigned)np), dim3(256), 0, g_stream, wit, cvec,
                  (const uint32_t*)bt->d_wit + first * (size_t)nv * 8, P->tail.as<uint32_t>(), L, mont ? 1u : 0u, bad,
                  P->grp_dev.as<uint32_t>(), pairs ? (const int32_t*)P->pairs_dev.as<int32_t>() : (const int32_t*)nullptr,
                  bytes ? P->sel_w.as<uint8_t>() : (uint8_t*)nullptr, bytes ? P->sel_c.as<uint8_t>() : (uint8_t*)nullptr, zkpairs::RUN_MAX);
        return ZK_OK;
    }

    // ---- multiexps (create_proof step 4).  The G2 job only needs the witness scalars: it is
    // enqueued first, on the side stream, and runs beside the H pipeline and the G1 multiexps (its
    // reduction tree is latency-bound with one job per proof; the G1 work fills the machine).
    zk_status g2_set() {
        const uint32_t wstride = plan.layout.wstride;
        P->jobs2.clear();
        for (size_t p = 0; p < np; p++) {
            MsmJob j2 = {wit + p * (size_t)wstride * 8, (pairs ? P->map_b2d : P->map_b2).as<int32_t>(), wstride, 0, (uint32_t)G2->n_points, 0, 0, 0};
            P->jobs2.push_back(j2);
        }
        HIP_TRY(hipEventRecord(g_ev_fork, g_stream));
        HIP_TRY(hipStreamWaitEvent(side, g_ev_fork, 0));
        // the bytes of the jobs' pair slots: the lengths of their terms pick the bases (msm.h MsmSelSet)
        const CJobLayout& L = plan.layout;
        zkdev::MsmSelSet sels = {};
        if (pairs && RUN_W) sels.r[0] = {P->sel_w.as<uint8_t>() + L.pa, P->alt_b2.as<int32_t>(), 0u, (uint32_t)np, L.sel_w, L.w_pair_b2, L.pb2, RUN_W};
        ZK_TRY(G2->enqueue(P->jobs2, P->res2, side, false, &sels));
        ZK_TRY(P->pin_g2.ensure(np * sizeof(HG2)));
        if (plan.host_norm) ZK_TRY(G2->export_to_host(G2->res_dev, np, P->pin_g2.as<HG2>(), P->fold_b2, side));
        else ZK_TRY(G2->normalize_to_host(G2->res_dev, np, P->pin_g2.as<HG2>(), P->fold_b2, side));   // B in affine form
        return ZK_OK;
    }

    // ---- H pipeline (create_proof step 3): the H block of every C job
    zk_status h_pipeline() {
        const size_t m = P->m;
        const uint32_t n_rows = bt->n_rows, cstride = plan.layout.cstride;
        ZK_TRY(P->abc.ensure((derived ? 2 : 3) * np * m * 32));
        uint32_t* A = P->abc.as<uint32_t>();
        uint32_t* B = A + np * m * 8;
        uint32_t* C = B + np * m * 8;
        const uint32_t* srcs[3] = {(const uint32_t*)bt->d_a + first * (size_t)n_rows * 8,
                                   (const uint32_t*)bt->d_b + first * (size_t)n_rows * 8,
                                   (const uint32_t*)bt->d_c + first * (size_t)n_rows * 8};
        uint32_t* dsts[3] = {A, B, C};
        // ifft (natural -> bit-reversed) of a and b, then * g^i / m (coset shift); c: * 1 / (m (g^m - 1)), plain - its
        // coefficients are all the H pipeline needs of c (ntt.h k_h_pointwise: 6 transforms per proof instead of bellman's 7).
        // Over the derived bases: a and b only, * t / m - the coefficients of x a'(x) - and the forward chain below is a plain
        // transform back onto the domain; the row evaluations themselves stay where they are (the chains load out of place).
        const uint32_t* s1 = derived ? P->ntt.dt.as<uint32_t>() : mont ? P->ntt.s1_mont.as<uint32_t>() : P->ntt.s1_plain.as<uint32_t>();
        const uint32_t* sc = mont ? P->ntt.sc_mont.as<uint32_t>() : P->ntt.sc_plain.as<uint32_t>();
        for (int k = 0; k < (derived ? 2 : 3); k++)
            ZK_TRY(P->ntt.chain(P->ntt.form((uint32_t)np), dsts[k], (uint32_t)np, (uint32_t)m, true, true, nullptr, k < 2 ? s1 : sc, srcs[k], n_rows, n_rows, bad));
        // (coset) fft (bit-reversed -> natural) of a and b at once
        ZK_TRY(P->ntt.chain(P->ntt.form((uint32_t)(2 * np)), A, (uint32_t)(2 * np), (uint32_t)m, false, false, nullptr, nullptr));
        {
            ProfScope ps("h_pointwise");
            if (derived) {
                // s_j and e_k of the live rows ARE the scalars (plain, natural order): four transforms per proof, none after this
                const size_t count = np * (size_t)n_rows;
                ZK_LAUNCH(zkdev::k_h_live_rows, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, g_stream, (const uint32_t*)A,
                          (const uint32_t*)B, srcs[0], srcs[1], srcs[2], cvec, (uint32_t)m, n_rows, cstride, count);
            } else {
                const size_t count = np * m;
                ZK_LAUNCH(zkdev::k_h_pointwise, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, g_stream, (const uint32_t*)A,
                          (const uint32_t*)B, (const uint32_t*)nullptr, P->ntt.consts.as<uint32_t>() + 8, cvec, (uint32_t)m, cstride, count);
            }
        }
        // icoset fft of a b / (g^m - 1): ifft (natural -> bit-reversed), * g^-i / m, Montgomery factor dropped, minus the
        // scaled coefficients of c (same bit-reversed order); in place inside the merged scalar vectors
        if (!derived)
            ZK_TRY(P->ntt.chain(P->ntt.form((uint32_t)np), cvec, (uint32_t)np, cstride, true, true, nullptr, P->ntt.s2.as<uint32_t>(), nullptr, 0, 0, nullptr,
                                (const uint32_t*)C, (uint32_t)m));
        return ZK_OK;
    }

    // ---- the G1 launch sets (prove_plan.h, split): the C' jobs on the main stream behind the H pipeline and the A jobs on the
    // side stream behind the G2 set, or one set on the main stream - all C' jobs, then all A jobs
    zk_status g1_sets() {
        const bool split = plan.split;
        const uint32_t wstride = plan.layout.wstride, cstride = plan.layout.cstride;
        const uint32_t npts1 = (uint32_t)P->g1.n_points, npts1c = (uint32_t)G1C->n_points;
        P->jobs1.clear();
        P->jobs1a.clear();
        for (size_t p = 0; p < np; p++) {
            MsmJob jc = {cvec + p * (size_t)cstride * 8, map_c, cstride, 0, npts1c, 0, 0, 0};
            P->jobs1.push_back(jc);
        }
        for (size_t p = 0; p < np; p++) {
            MsmJob ja = {wit + p * (size_t)wstride * 8, P->map_a.as<int32_t>(), wstride, P->off_a, npts1, 0, 0, 0};
            if (pairs) {   // (absolute positions in the derived table: the pair bases lie in front of its copy of the A query)
                ja.map = P->map_ad.as<int32_t>();
                ja.table_base = 0;
                ja.n_table = (uint32_t)P->g1d.n_points;
            } else if (!split && derived) {   // (one set with the C' jobs: the A query's copy behind the derived bases)
                ja.table_base = P->drv.off_a;
                ja.n_table = npts1c;
            }
            (split ? P->jobs1a : P->jobs1).push_back(ja);
        }
        // the ranges of jobs whose pair slots follow the bytes (msm.h MsmSelSet): the C' jobs, the A jobs
        const CJobLayout& L = plan.layout;
        zkdev::MsmSelSet sc = {}, sa = {};
        if (pairs && RUN_W) {
            sc.r[0] = {P->sel_c.as<uint8_t>(), P->alt_c.as<int32_t>(), 0u, (uint32_t)np, L.sel_c, L.pair_l, L.sel_c, RUN_W};
            sa.r[0] = {P->sel_w.as<uint8_t>(), P->alt_a.as<int32_t>(), 0u, (uint32_t)np, L.sel_w, L.w_pair_a, L.pa, RUN_W};
            if (!split) {   // (one set: the A jobs behind the C' jobs)
                sc.r[1] = sa.r[0];
                sc.r[1].job0 = (uint32_t)np;
            }
        }
        if (split) {
            MsmG1& G1A = pairs ? P->g1da : P->g1a;
            ZK_TRY(G1A.enqueue(P->jobs1a, P->res1a, side, false, &sa));
            a_dev = G1A.res_dev;
            HIP_TRY(hipEventRecord(g_ev_join, side));
            ZK_TRY(G1C->enqueue(P->jobs1, P->res1, g_stream, false, &sc));
            HIP_TRY(hipStreamWaitEvent(g_stream, g_ev_join, 0));   // (a no-op when the side stream is the main one)
        } else {
            ZK_TRY(G1C->enqueue(P->jobs1, P->res1, g_stream, false, &sc));
            a_dev = G1C->res_dev + np;
        }
        return ZK_OK;
    }

    // ---- final fold on the GPU: C = s * A + C' (coop_tail.h scale_add), A and C to affine form; the host
    // only encodes.  (On the host the fold was 0.47 ms per proof with the GPU idle: 8 % of the step.)
    zk_status fold_export() {
        ProfScope ps("proof_fold", g_stream);
        const DP1* cprime = G1C->res_dev;
        const DP1* cfin = cprime;   // the C job was s * A + C' already
        if (!plan.fold_in_msm) {
            ZK_TRY(P->fold_tbl.ensure(np * 15 * sizeof(DP1)));
            ZK_TRY(P->fold_c.ensure(np * sizeof(DP1)));
            // one row of 16 lanes per proof (coop_tail.cpp): 256 waves, each chain 4 - 5 x shorter than a lane's
            zkcoop::scale_add(a_dev, cprime, (const uint32_t*)P->tail.as<uint32_t>() + 16, 24u, P->fold_tbl.as<DP1>(),
                              P->fold_c.as<DP1>(), (uint32_t)np, g_stream);
            cfin = P->fold_c.as<DP1>();
        }
        ZK_TRY(P->pin_g1.ensure(2 * np * sizeof(HG1)));
        if (plan.host_norm) {
            ZK_TRY(G1C->export_to_host(a_dev, np, P->pin_g1.as<HG1>() + np, P->fold_a1, g_stream));
            ZK_TRY(G1C->export_to_host(cfin, np, P->pin_g1.as<HG1>(), P->fold_c1, g_stream));
        } else {
            ZK_TRY(G1C->normalize2_to_host(a_dev, cfin, np, P->pin_g1.as<HG1>() + np, P->pin_g1.as<HG1>(), P->fold_a1, P->fold_c1, g_stream));
        }
        return ZK_OK;
    }

    // ---- wait for the GPU; the flags the kernels raised over the caller's scalars
    zk_status collect(std::chrono::steady_clock::time_point& t_wait) {
        HIP_TRY(hipMemcpyAsync(P->pin_bad.p, bad, 8, hipMemcpyDeviceToHost, g_stream));
        t_wait = std::chrono::steady_clock::now();
        ZK_TRY(G1C->collect(g_stream));
        ZK_TRY(G2->collect(side));
        // the reference cannot even represent these assignments (FrRepr -> Fr fails for values >= r,
        // fr.rs:276-289; ProvingAssignment starts with alloc_input(ONE = 1))
        const uint32_t flags = P->pin_bad.as<uint32_t>()[0];
        if (flags & zkdev::ZK_BAD_SCALAR)
            return fail(ZK_ERR_INVALID_ARGUMENT, "an assignment scalar (a, b, c, input or aux) is not a canonical field element (>= r)");
        if (flags & zkdev::ZK_BAD_ONE) return fail(ZK_ERR_INVALID_ARGUMENT, "input 0 of an assignment is not ONE = 1");
        return ZK_OK;
    }

    // ---- encoding (host, one thread per slice of the chunk): pin_g1[p] = C, pin_g1[np + p] = A, pin_g2[p] = B
    void encode(uint8_t* proofs_out) {
        const unsigned nthreads = host_threads(np, 32);
        uint8_t* const own_affine = g_own_affine_sink;   // (read on the calling thread: the workers below are other threads)
        auto work = [&](size_t lo, size_t hi) {
            for (size_t p = lo; p < hi; p++)
            {
                uint8_t* out = proofs_out + (first + p) * 192;
                const HG1A pa = zkhost::to_affine(P->pin_g1.as<HG1>()[np + p]), pc = zkhost::to_affine(P->pin_g1.as<HG1>()[p]);
                const HG2A pb = zkhost::to_affine(P->pin_g2.as<HG2>()[p]);
                zkhost::g1_to_compressed(pa, out);
                zkhost::g2_to_compressed(pb, out + 48);
                zkhost::g1_to_compressed(pc, out + 144);
                if (own_affine) {   // for the self-check of gen_proof (host_common.h g_own_affine_sink)
                    uint8_t* o = own_affine + p * OWN_AFFINE_BYTES;   // (a cursor: the chunks of a call arrive in order)
                    memcpy(o, &pa.x, 48);
                    memcpy(o + 48, &pa.y, 48);
                    memcpy(o + 96, &pb.x, 96);
                    memcpy(o + 192, &pb.y, 96);
                    memcpy(o + 288, &pc.x, 48);
                    memcpy(o + 336, &pc.y, 48);
                }
            }
        };
        auto part = [&](unsigned t) { work(np * t / nthreads, np * (t + 1) / nthreads); };
        run_threads(nthreads, part);
        if (g_own_affine_sink) g_own_affine_sink += np * OWN_AFFINE_BYTES;
    }
};

zk_status prove_chunk(zk_params* P, size_t np, const zk_batch_dev* bt, size_t first, const uint8_t* rs, uint8_t* proofs_out, bool derived) {
    const auto t_begin = std::chrono::steady_clock::now();
    const ProveTunables tun = ProveTunables::read();
    const bool mont = (bt->flags & ZK_FR_MONTGOMERY) != 0;
    if (derived && (!mont || P->drv.n_rows != bt->n_rows)) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: the batch is not the derived set's");
    ChunkRun c = {P, np, bt, first, derived, mont,
                  prove_plan(np, bt->n_inputs, bt->n_aux, bt->n_rows, P->m, P->mg_a, P->mg_b2, P->mg_b1, derived, tun, P->mpairs)};
    c.pairs = c.plan.layout.w_b2v != 0;
    c.side = c.plan.one_stream ? g_stream : g_stream2;
    c.G2 = c.pairs ? (c.plan.g2_lone ? &P->g2p_lone : &P->g2p) : (c.plan.g2_lone ? &P->g2_lone : &P->g2);
    MsmG1* const g1s[] = {&P->g1, &P->g1_lone, &P->g1d, &P->g1d_lone};   // in the order of PG1 and PMap
    DevBuf* const maps[] = {&P->map_c, &P->map_cf, &P->map_cd, &P->map_cfd};
    c.G1C = g1s[(int)c.plan.g1];
    c.map_c = maps[(int)c.plan.map]->as<int32_t>();
    ZK_TRY(c.scalars(rs));
    ZK_TRY(c.g2_set());
    ZK_TRY(c.h_pipeline());
    ZK_TRY(c.g1_sets());
    ZK_TRY(c.fold_export());
    std::chrono::steady_clock::time_point t_wait;
    ZK_TRY(c.collect(t_wait));
    const auto t_enc = std::chrono::steady_clock::now();
    c.encode(proofs_out);
    if (tun.trace_host) {
        const auto t_end = std::chrono::steady_clock::now();
        fprintf(stderr, "[zkamd] chunk of %zu: enqueue %.2f ms, wait for the GPU %.2f ms, host encoding %.2f ms\n", np,
                std::chrono::duration<double, std::milli>(t_wait - t_begin).count(),
                std::chrono::duration<double, std::milli>(t_enc - t_wait).count(),
                std::chrono::duration<double, std::milli>(t_end - t_enc).count());
        // the (digit, point) pairs of the chunk's launch sets, counted from their buckets
        uint64_t pc1 = 0, pa1 = 0, p2 = 0;
        ZK_TRY(c.G1C->count_pairs(c.plan.split ? np : 2 * np, &pc1));
        if (c.plan.split) ZK_TRY((c.pairs ? P->g1da : P->g1a).count_pairs(np, &pa1));
        ZK_TRY(c.G2->count_pairs(np, &p2));
        fprintf(stderr, "[zkamd] chunk of %zu: pairs per proof: %s %.0f, A set %.0f, G2 set %.0f\n", np, c.plan.split ? "C' set" : "C' and A set",
                (double)pc1 / (double)np, (double)pa1 / (double)np, (double)p2 / (double)np);
    }
    return ZK_OK;
}

zk_status prove_batch_dev(zk_params* P, size_t n, const zk_batch_dev* bt, const uint8_t* rs, uint8_t* proofs_out, bool derived = false) {
    if (!P || !bt || !rs || !proofs_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(P->device));
    // bellman create_proof: `if vk.delta_g1.is_zero() || vk.delta_g2.is_zero() { return Err(UnexpectedIdentity) }`
    if (P->delta_g1_inf || P->delta_g2_inf) return fail(ZK_ERR_UNEXPECTED_IDENTITY, "vk.delta is the point at infinity");
    if (bt->n_inputs == 0) return fail(ZK_ERR_INVALID_ARGUMENT, "n_inputs must include ONE");
    if (bt->n_rows > P->m) return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    if (bt->n_inputs != P->n_ic) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "number of inputs differs from vk.ic");
    if (bt->n_aux != P->n_l) return fail(ZK_ERR_IO, "number of aux variables differs from the l query");
    if (!bt->d_a || !bt->d_b || !bt->d_c || !bt->d_wit || !bt->a_aux_density || !bt->b_input_density || !bt->b_aux_density)
        return fail(ZK_ERR_ASSIGNMENT_MISSING, "assignment pointer is null");
    ZK_TRY(ensure_maps(P, bt->n_inputs, bt->n_aux, bt->a_aux_density, bt->b_input_density, bt->b_aux_density));
    const size_t chunk = ProveTunables::read().batch_chunk;
    for (size_t first = 0; first < n; first += chunk) {
        size_t np = std::min(chunk, n - first);
        ZK_TRY(prove_chunk(P, np, bt, first, rs, proofs_out, derived));
    }
    return ZK_OK;
}

bool same_circuit(const zk_assignment& x, const zk_assignment& y) {
    return x.n_rows == y.n_rows && x.n_inputs == y.n_inputs && x.n_aux == y.n_aux && x.flags == y.flags &&
           memcmp(x.a_aux_density, y.a_aux_density, x.n_aux) == 0 &&
           memcmp(x.b_input_density, y.b_input_density, x.n_inputs) == 0 &&
           memcmp(x.b_aux_density, y.b_aux_density, x.n_aux) == 0;
}

zk_status prove_batch_host(zk_params* P, size_t n, const zk_assignment* asgs, const uint8_t* rs, uint8_t* proofs_out) {
    if (!P || !asgs || !rs || !proofs_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(P->device));
    const zk_assignment& z = asgs[0];
    for (size_t i = 0; i < n; i++) {
        const zk_assignment& x = asgs[i];
        if (!x.a || !x.b || !x.c || !x.inputs || !x.aux || !x.a_aux_density || !x.b_input_density || !x.b_aux_density)
            return fail(ZK_ERR_ASSIGNMENT_MISSING, "assignment pointer is null");
        if (i && !same_circuit(z, x)) return fail(ZK_ERR_INVALID_ARGUMENT, "batch mixes different circuits");
    }
    const size_t rb = (size_t)z.n_rows * 32, nvb = (size_t)(z.n_inputs + z.n_aux) * 32;
    // The assignments (2.6 MB per Transfer proof) cross PCIe in blocks: block k + 1 is staged by a
    // helper thread on its own stream while the GPU proves block k out of the other half of the
    // staging buffers.  A batch that fits one device chunk is cut in two halves so that only the first
    // half's copy is exposed (measured on 1024 Transfer proofs: whole 2101, halves 2240, quarters 2119
    // proofs/s - smaller launch sets lose more in the kernels than the hidden copy gains).
    const ProveTunables tun = ProveTunables::read();
    const size_t chunk = tun.batch_chunk;
    size_t hc = n > chunk ? chunk : (n >= 512 ? (n + 1) / 2 : n);
    if (tun.host_chunk) hc = std::min(chunk, tun.host_chunk);
    hc = std::min(hc, n);
    const size_t slots = n > hc ? 2 : 1;
    ZK_TRY(P->stage_a.ensure(slots * hc * rb));
    ZK_TRY(P->stage_b.ensure(slots * hc * rb));
    ZK_TRY(P->stage_c.ensure(slots * hc * rb));
    ZK_TRY(P->stage_w.ensure(slots * hc * nvb));
    const hipStream_t copy_stream = g_copy_stream;   // thread-local view: the helper thread gets it by value
    auto stage = [&, copy_stream](size_t slot, size_t first, size_t np) -> zk_status {
        HIP_TRY(hipSetDevice(P->device));   // the current device is per host thread
        uint8_t* da = (uint8_t*)P->stage_a.p + slot * hc * rb;
        uint8_t* db = (uint8_t*)P->stage_b.p + slot * hc * rb;
        uint8_t* dc = (uint8_t*)P->stage_c.p + slot * hc * rb;
        uint8_t* dw = (uint8_t*)P->stage_w.p + slot * hc * nvb;
        for (size_t i = 0; i < np; i++) {
            const zk_assignment& x = asgs[first + i];
            HIP_TRY(hipMemcpyAsync(da + i * rb, x.a, rb, hipMemcpyHostToDevice, copy_stream));
            HIP_TRY(hipMemcpyAsync(db + i * rb, x.b, rb, hipMemcpyHostToDevice, copy_stream));
            HIP_TRY(hipMemcpyAsync(dc + i * rb, x.c, rb, hipMemcpyHostToDevice, copy_stream));
            HIP_TRY(hipMemcpyAsync(dw + i * nvb, x.inputs, (size_t)z.n_inputs * 32, hipMemcpyHostToDevice, copy_stream));
            HIP_TRY(hipMemcpyAsync(dw + i * nvb + (size_t)z.n_inputs * 32, x.aux, (size_t)z.n_aux * 32, hipMemcpyHostToDevice,
                                   copy_stream));
        }
        HIP_TRY(hipStreamSynchronize(copy_stream));
        return ZK_OK;
    };
    ZK_TRY(stage(0, 0, hc));
    size_t cur = 0;
    for (size_t first = 0; first < n; first += hc) {
        const size_t np = std::min(hc, n - first), next = first + hc;
        zk_status next_rc = ZK_OK;
        std::string next_err;
        SideThread copier;
        if (next < n)
            copier.start([&, next] {
                next_rc = stage(cur ^ 1, next, std::min(hc, n - next));
                if (next_rc != ZK_OK) next_err = g_err;   // g_err is thread-local
            });
        zk_batch_dev bt;
        bt.n_rows = z.n_rows;
        bt.n_inputs = z.n_inputs;
        bt.n_aux = z.n_aux;
        bt.flags = z.flags;
        bt.d_a = (uint8_t*)P->stage_a.p + cur * hc * rb;
        bt.d_b = (uint8_t*)P->stage_b.p + cur * hc * rb;
        bt.d_c = (uint8_t*)P->stage_c.p + cur * hc * rb;
        bt.d_wit = (uint8_t*)P->stage_w.p + cur * hc * nvb;
        bt.a_aux_density = z.a_aux_density;
        bt.b_input_density = z.b_input_density;
        bt.b_aux_density = z.b_aux_density;
        zk_status rc = prove_batch_dev(P, np, &bt, rs + first * 64, proofs_out + first * 192);
        copier.join();
        if (rc != ZK_OK) return rc;
        if (next_rc != ZK_OK) return fail(next_rc, next_err);
        cur ^= 1;
    }
    return ZK_OK;
}

}  // namespace

namespace {

zk_status r1cs_load(uint32_t n_in, uint32_t n_aux, uint32_t n_con, const zk_csr* const mats[3], int device, zk_r1cs** out) {
    ZK_TRY(use_device(device));
    if (n_in == 0) return fail(ZK_ERR_INVALID_ARGUMENT, "n_inputs must include ONE");
    zk_r1cs* R = new (std::nothrow) zk_r1cs();
    if (!R) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    struct Guard {
        zk_r1cs* p;
        ~Guard() { delete p; }
    } guard{R};
    R->device = device;
    static std::atomic<uint64_t> next_id{1};
    R->id = next_id++;
    R->n_in = n_in;
    R->n_aux = n_aux;
    R->n_con = n_con;
    const uint32_t nv = n_in + n_aux;
    R->a_aux_density.assign(n_aux, 0);
    R->b_input_density.assign(n_in, 0);
    R->b_aux_density.assign(n_aux, 0);
    for (int m = 0; m < 3; m++) {
        const zk_csr* M = mats[m];
        if (!M || !M->row_ptr || (n_con && M->row_ptr[n_con] && (!M->col || !M->coeff)))
            return fail(ZK_ERR_INVALID_ARGUMENT, "null matrix pointer");
        if (M->row_ptr[0] != 0) return fail(ZK_ERR_INVALID_ARGUMENT, "row_ptr[0] must be 0");
        for (uint32_t r = 0; r < n_con; r++)
            if (M->row_ptr[r + 1] < M->row_ptr[r]) return fail(ZK_ERR_INVALID_ARGUMENT, "row_ptr is not monotone");
        const uint32_t nnz = M->row_ptr[n_con];
        for (uint32_t k = 0; k < nnz; k++) {
            const uint32_t v = M->col[k];
            if (v >= nv) return fail(ZK_ERR_INVALID_ARGUMENT, "variable index out of range in matrix " + std::to_string(m));
            uint64_t c[4];
            load_scalar_le(M->coeff + (size_t)k * 32, c);
            if (!scalar_lt_r(c)) return fail(ZK_ERR_INVALID_ARGUMENT, "coefficient is not < r");
            // bellman's density trackers: a variable counts as soon as it APPEARS in a row of A / B
            if (m == 0 && v >= n_in) R->a_aux_density[v - n_in] = 1;
            if (m == 1) {
                if (v >= n_in)
                    R->b_aux_density[v - n_in] = 1;
                else
                    R->b_input_density[v] = 1;
            }
        }
        R->h_row_ptr[m].assign(M->row_ptr, M->row_ptr + n_con + 1);
        R->h_col[m].assign(M->col, M->col + nnz);
        R->h_coeff[m].resize(nnz);
        for (uint32_t k = 0; k < nnz; k++) {
            zkhost::Fr c;
            load_scalar_le(M->coeff + (size_t)k * 32, c.l);
            R->h_coeff[m][k] = c.to_mont();
        }
        ZK_TRY(R->row_ptr[m].ensure(((size_t)n_con + 1) * 4));
        ZK_TRY(R->col[m].ensure((size_t)(nnz ? nnz : 1) * 4));
        ZK_TRY(R->coeff[m].ensure((size_t)(nnz ? nnz : 1) * 32));
        HIP_TRY(hipMemcpy(R->row_ptr[m].p, M->row_ptr, ((size_t)n_con + 1) * 4, hipMemcpyHostToDevice));
        if (nnz) {
            HIP_TRY(hipMemcpy(R->col[m].p, M->col, (size_t)nnz * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(R->coeff[m].p, M->coeff, (size_t)nnz * 32, hipMemcpyHostToDevice));
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((nnz + 255) / 256), dim3(256), 0, g_stream, R->coeff[m].as<uint32_t>(),
                      (const uint32_t*)R->coeff[m].as<uint32_t>(), 0u, (size_t)nnz);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    guard.p = nullptr;
    *out = R;
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
// their terms).  Fills P->prs but for where the bases lie; a circuit without built-in probes has no pairs.
// the natively emitted constraint systems of the two built-in circuits (transfer_r1cs.h), each built once per process
const zkr1cs::System& builtin_system(zkpairs::Circuit c) {
    if (c == zkpairs::TRANSFER) {
        static const zkr1cs::System sys = zkr1cs::transfer_system();
        return sys;
    }
    static const zkr1cs::System sys = zkr1cs::anonymous_system();
    return sys;
}
struct PairBases {
    std::vector<HG1A> l, b1, a;
    std::vector<HG2A> b2;
    std::vector<HG1A> xl, xb1, xa;   // the longer runs' (value_pairs.h RUN_MAX), behind all of the above
    std::vector<HG2A> xb2;
};
template <class A>
A sum_of_two(const A& x, const A& y) {
    typedef decltype(x.x) F;
    return zkhost::to_affine(zkhost::padd(zkhost::Point<F>::from_affine(x), zkhost::Point<F>::from_affine(y)));
}
void derived_pairs(zk_params* P, const zk_r1cs* R, const std::vector<HG1A>& set, uint32_t n_rows, PairBases& out) {
    zk_params::Pairs& X = P->prs;
    X = zk_params::Pairs();
    const uint32_t n_in = R->n_in, n_aux = R->n_aux, nv = n_in + n_aux;
    zkpairs::Circuit kind;
    if (n_in == ZK_TRANSFER_N_INPUTS && n_aux == ZK_TRANSFER_N_AUX) kind = zkpairs::TRANSFER;
    else if (n_in == ZK_ANONYMOUS_N_INPUTS && n_aux == ZK_ANONYMOUS_N_AUX) kind = zkpairs::ANONYMOUS;
    else return;
    if (P->enc_a.size() != (size_t)P->n_a * 96 || P->enc_b1.size() != (size_t)P->n_b1 * 96 || P->enc_b2.size() != (size_t)P->n_b2 * 192) return;
    std::vector<uint8_t> a_dense(nv, 1), b_dense(nv, 0);
    for (uint32_t i = 0; i < nv; i++) {
        if (i >= n_in) a_dense[i] = R->a_aux_density[i - n_in];
        b_dense[i] = i < n_in ? R->b_input_density[i] : R->b_aux_density[i - n_in];
    }
    {
        // The probes are witnesses of the BUILT-IN circuit: another circuit with its counts would get chains that merge nothing
        // and pay for their bases and tables.  The caller's matrices must have the built-in system's constraint count and
        // densities (which variables occur in A and in B) - what the chains are made from.
        const zkr1cs::System& sys = builtin_system(kind);
        if (sys.n_inputs != n_in || sys.n_aux != n_aux || sys.n_constraints != R->n_con) return;
        std::vector<uint8_t> sa(nv, 0), sb(nv, 0);
        for (uint32_t i = 0; i < n_in; i++) sa[i] = 1;
        for (uint32_t v : sys.m[0].col) sa[v] = 1;
        for (uint32_t v : sys.m[1].col) sb[v] = 1;
        if (sa != a_dense || sb != b_dense) return;
    }
    const std::vector<std::vector<Fr>>& probes = zkpairs::circuit_probes(kind);
    if (probes.empty() || probes[0].size() != nv || set.size() != 2 * (size_t)n_rows + nv) return;
    // [pred A | succ A | pred B | succ B | pred L | succ L]
    const std::vector<int32_t> chains = zkpairs::chains_of(probes, n_in, a_dense, b_dense);
    const int32_t *pred_a = chains.data(), *pred_b = pred_a + 2 * (size_t)nv, *pred_l = pred_a + 4 * (size_t)nv;
    // variable -> position in the A query / the B queries / the set, -1 where it has no term
    std::vector<int32_t> pa(nv, -1), pb1(nv, -1), pb2(nv, -1), pl(nv, -1);
    uint32_t at = 0;
    for (uint32_t i = 0; i < nv; i++)
        if (i < n_in || R->a_aux_density[i - n_in]) pa[i] = (int32_t)at++;
    if (at != P->n_a) return;
    at = 0;
    for (uint32_t i = 0; i < nv; i++)
        if (i < n_in ? R->b_input_density[i] : R->b_aux_density[i - n_in]) pb1[i] = pb2[i] = (int32_t)at++;
    if (at != P->n_b1 || at != P->n_b2) return;
    for (uint32_t i = n_in; i < nv; i++)
        if (!set[2 * (size_t)n_rows + i].is_inf()) pl[i] = (int32_t)(2 * n_rows + i);
    struct Cand {
        uint32_t j;
        int32_t p, q;   // positions of the two bases
    };
    std::vector<Cand> ca, cb1, cb2, cl;
    for (uint32_t j = 0; j < nv; j++) {
        int32_t p = pred_a[j];
        if (p >= 0 && pa[j] >= 0 && pa[p] >= 0) ca.push_back({j, pa[p], pa[j]});
        p = pred_b[j];
        if (p >= 0 && pb1[j] >= 0 && pb1[p] >= 0) cb1.push_back({j, pb1[p], pb1[j]});
        if (p >= 0 && pb2[j] >= 0 && pb2[p] >= 0) cb2.push_back({j, pb2[p], pb2[j]});
        p = pred_l[j];
        if (p >= 0 && pl[j] >= 0 && pl[p] >= 0) cl.push_back({j, pl[p], pl[j]});
    }
    std::vector<HG1A> sa(ca.size()), sb1(cb1.size()), sl(cl.size());
    std::vector<HG2A> sb2(cb2.size());
    auto g1_at = [](const std::vector<uint8_t>& enc, int32_t pos) {
        HG1A pt = HG1A::inf();
        if (zkhost::g1_from_uncompressed(enc.data() + (size_t)pos * 96, &pt) != zkhost::DEC_OK) pt = HG1A::inf();
        return pt;
    };
    auto g2_at = [](const std::vector<uint8_t>& enc, int32_t pos) {
        HG2A pt = HG2A::inf();
        if (zkhost::g2_from_uncompressed(enc.data() + (size_t)pos * 192, &pt) != zkhost::DEC_OK) pt = HG2A::inf();
        return pt;
    };
    const size_t total = ca.size() + cb1.size() + cb2.size() + cl.size();
    const unsigned nthreads = host_threads(total / 64 + 1, 32);
    auto part = [&](unsigned t) {
        auto range = [&](size_t n, auto&& fn) {
            for (size_t k = n * t / nthreads; k < n * (t + 1) / nthreads; k++) fn(k);
        };
        range(ca.size(), [&](size_t k) { sa[k] = sum_of_two(g1_at(P->enc_a, ca[k].p), g1_at(P->enc_a, ca[k].q)); });
        range(cb1.size(), [&](size_t k) { sb1[k] = sum_of_two(g1_at(P->enc_b1, cb1[k].p), g1_at(P->enc_b1, cb1[k].q)); });
        range(cb2.size(), [&](size_t k) { sb2[k] = sum_of_two(g2_at(P->enc_b2, cb2[k].p), g2_at(P->enc_b2, cb2[k].q)); });
        range(cl.size(), [&](size_t k) { sl[k] = sum_of_two(set[cl[k].p], set[cl[k].q]); });
    };
    run_threads(nthreads, part);
    // links = [the chains | qa | qb2 | ql | qb1]
    X.links.assign(11 * (size_t)nv, -1);
    std::copy(chains.begin(), chains.end(), X.links.begin());
    std::fill(X.links.begin() + 10 * (size_t)nv, X.links.end(), 0);   // (the bits of the longer bases, below)
    auto keep = [&](const std::vector<Cand>& c, const auto& sums, auto& bases, int32_t* q) {
        for (size_t k = 0; k < c.size(); k++)
            if (!sums[k].is_inf()) {
                q[c[k].j] = (int32_t)bases.size();
                bases.push_back(sums[k]);
            }
        return (uint32_t)bases.size();
    };
    int32_t* q = &X.links[6 * (size_t)nv];
    X.n.a = keep(ca, sa, out.a, q);
    X.n.b2 = keep(cb2, sb2, out.b2, q + nv);
    X.n.l = keep(cl, sl, out.l, q + 2 * (size_t)nv);
    X.n.b1 = keep(cb1, sb1, out.b1, q + 3 * (size_t)nv);
    // The longer runs: for every link j that has its pair base and l = 3 ... RUN_MAX, the sum of the l chain members that end at
    // j, as long as the links behind it have their pair bases.  The thread of j walks back from j, adding one member per length
    // (so P_j + P_pred is added again, per link) and normalises every length it keeps (an inversion each): 49 ms of binding for
    // the transfer key at 4.  A sum that comes out as the identity has no base and no bit: k_build_scalars then splits the run
    // into shorter terms.
    int32_t* const avail = &X.links[10 * (size_t)nv];
    auto longer = [&](uint32_t query, uint32_t n_pairs, const int32_t* pred, const int32_t* qq, const std::vector<int32_t>& pos, auto&& point,
                      auto& bases) {
        typedef typename std::decay_t<decltype(bases)>::value_type A;
        typedef decltype(A().x) F;
        constexpr uint32_t W = zkpairs::RUN_MAX - 2;
        X.alt[query].assign((size_t)n_pairs * W, -1);
        if (!W) return;
        std::vector<uint32_t> js;
        for (uint32_t j = 0; j < nv; j++)
            if (qq[j] >= 0 && qq[pred[j]] >= 0) js.push_back(j);
        std::vector<A> sums(js.size() * W, A::inf());
        const unsigned nt = host_threads(js.size() / 64 + 1, 32);
        auto work = [&](unsigned t) {
            for (size_t k = js.size() * t / nt; k < js.size() * (t + 1) / nt; k++) {
                const uint32_t j = js[k];
                int32_t cur = pred[j];
                auto acc = zkhost::padd(zkhost::Point<F>::from_affine(point(pos[j])), zkhost::Point<F>::from_affine(point(pos[cur])));
                for (uint32_t l = 3; l <= zkpairs::RUN_MAX && qq[cur] >= 0; l++) {
                    cur = pred[cur];
                    acc = zkhost::padd(acc, zkhost::Point<F>::from_affine(point(pos[cur])));
                    sums[k * W + (l - 3)] = zkhost::to_affine(acc);
                }
            }
        };
        run_threads(nt, work);
        for (size_t k = 0; k < js.size(); k++)
            for (uint32_t l = 3; l <= zkpairs::RUN_MAX; l++)
                if (!sums[k * W + (l - 3)].is_inf()) {
                    X.alt[query][(size_t)qq[js[k]] * W + (l - 3)] = (int32_t)bases.size();
                    bases.push_back(sums[k * W + (l - 3)]);
                    avail[js[k]] |= (int32_t)(1u << (8 * query + (l - 1)));
                    X.xn[query][l - 3]++;
                }
    };
    longer(0, X.n.a, pred_a, q, pa, [&](int32_t at) { return g1_at(P->enc_a, at); }, out.xa);
    longer(1, X.n.b2, pred_b, q + nv, pb2, [&](int32_t at) { return g2_at(P->enc_b2, at); }, out.xb2);
    longer(2, X.n.l, pred_l, q + 2 * (size_t)nv, pl, [&](int32_t at) { return set[at]; }, out.xl);
    longer(3, X.n.b1, pred_b, q + 3 * (size_t)nv, pb1, [&](int32_t at) { return g1_at(P->enc_b1, at); }, out.xb1);
    // what a proof is expected to merge, from the probes
    uint64_t merged[4] = {0, 0, 0, 0};
    for (const std::vector<Fr>& z : probes) {
        merged[0] += zkpairs::count_merges(pred_a, pred_a + nv, q, avail, 0, z);
        merged[1] += zkpairs::count_merges(pred_b, pred_b + nv, q + nv, avail, 1, z);
        merged[2] += zkpairs::count_merges(pred_l, pred_l + nv, q + 2 * (size_t)nv, avail, 2, z);
        merged[3] += zkpairs::count_merges(pred_b, pred_b + nv, q + 3 * (size_t)nv, avail, 3, z);
    }
    const uint64_t np = probes.size();
    X.exp_a = (uint32_t)(merged[0] / np);
    X.exp_b2 = (uint32_t)(merged[1] / np);
    X.exp_l = (uint32_t)(merged[2] / np);
    X.exp_b1 = (uint32_t)(merged[3] / np);
    X.ready = X.n.any();
}

zk_status ensure_derived(zk_params* P, zk_r1cs* R) {
    if (P->drv.ready && P->drv.circuit == R->id) return ZK_OK;
    const uint32_t n_in = R->n_in, n_aux = R->n_aux, nv = n_in + n_aux, n_con = R->n_con, n_rows = n_con + n_in, k = P->log_m;
    const size_t m = P->m;
    if (!P->g1.table.owned || R->h_row_ptr[2].size() != (size_t)n_con + 1 || n_in != P->n_ic || n_aux != P->n_l ||
        (size_t)n_con + n_in > m || P->n_h + 1 != m)
        return ZK_OK;
    ZK_TRY(use_device(P->device));
    const auto t0 = std::chrono::steady_clock::now();
    typedef zkdev::XYZZ<zkdev::Fq> DP;
    typedef zkdev::Affine<zkdev::Fq> DA;
    P->drv.ready = false;
    const DA* key = P->g1.table.as<DA>();
    // C by columns, the coefficients in plain words
    const std::vector<uint32_t>& rp = R->h_row_ptr[2];
    const std::vector<uint32_t>& cl = R->h_col[2];
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
                t_s[slot] = R->h_coeff[2][e].from_mont();
            }
    }
    for (uint32_t i = 0; i <= n_rows; i++) each[i] = i;   // (segments of one term: E_k = M_k + one point)
    // H in bit-reversed order with the identity in the place of H_(m-1); the L query behind the (empty) inputs
    std::vector<int32_t> idx(m + nv);
    for (size_t pos = 0; pos < m; pos++) {
        const uint32_t e = k ? (__builtin_bitreverse32((uint32_t)pos) >> (32 - k)) : 0;
        idx[pos] = e < P->n_h ? (int32_t)(P->off_h + e) : -1;
    }
    for (uint32_t i = 0; i < nv; i++) idx[m + i] = i < n_in ? -1 : (int32_t)(P->off_l + (i - n_in));
    const size_t rows = std::max<size_t>(m, nnz), n_set = 2 * (size_t)n_rows + nv;
    DevBuf d_idx, d_ptr, d_each, d_row, d_s, d_tw, d_w, d_sl, d_sm, d_se, src, ping, pong, lam, mk, terms, tbl, all, stage;
    for (DevBuf* b : {&d_idx, &d_ptr, &d_each, &d_row, &d_s, &d_tw, &d_w, &d_sl, &d_sm, &d_se, &src, &ping, &pong, &lam, &mk, &terms, &tbl, &all, &stage})
        b->is_public = true;
    ZK_TRY(d_idx.ensure(idx.size() * 4));
    ZK_TRY(d_ptr.ensure(ptr.size() * 4));
    ZK_TRY(d_each.ensure(each.size() * 4));
    ZK_TRY(d_row.ensure(t_row.size() * 4));
    ZK_TRY(d_s.ensure(t_s.size() * 32));
    ZK_TRY(d_tw.ensure(m * 32));
    ZK_TRY(d_w.ensure(5 * 32));
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
    HIP_TRY(hipMemcpy(d_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ptr.p, ptr.data(), ptr.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_each.p, each.data(), each.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_row.p, t_row.data(), t_row.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s.p, t_s.data(), t_s.size() * 32, hipMemcpyHostToDevice));
    const Fr ninv2 = P->ntt.n_inv * P->ntt.n_inv;
    const Fr wv[5] = {P->ntt.w_inv, Fr::one(), ninv2, -ninv2, fr_from_u64((uint64_t)m) * P->ntt.z_inv};
    HIP_TRY(hipMemcpy(d_w.p, wv, sizeof(wv), hipMemcpyHostToDevice));
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
    ZK_TRY(P->g1.normalize_to_host(set, n_set, host.data(), stage, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    std::vector<HG1A> pts(n_set);
    P->drv.pos.assign(n_set, -1);
    size_t live = 0;
    for (size_t i = 0; i < n_set; i++) {
        pts[i] = host[i].is_inf() ? HG1A::inf() : HG1A{host[i].x, host[i].y};
        if (!host[i].is_inf()) {
            P->drv.pos[i] = (int32_t)i;
            if (i < n_rows || i >= 2 * (size_t)n_rows) live++;
        }
    }
    // (the width of the set's own terms: the residuals are zero scalars unless a constraint fails)
    // value pairs: [pairs of the L terms | of the B1 query | of the A query] behind the set, the B2 query's in a table of its own.
    // A set expects fewer terms per proof with them (the mean over the probes), and its width follows that.
    PairBases pb;
    derived_pairs(P, R, pts, n_rows, pb);
    zk_params::Pairs& X = P->prs;
    X.base_l = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.l.begin(), pb.l.end());
    X.base_b1 = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.b1.begin(), pb.b1.end());
    X.base_a = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.a.begin(), pb.a.end());
    X.base_b2 = P->n_b2 + 2;
    // (the longer runs' bases behind every pair section: the pair sections stay where a set without them has them)
    X.xbase[2] = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.xl.begin(), pb.xl.end());
    X.xbase[3] = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.xb1.begin(), pb.xb1.end());
    X.xbase[0] = (uint32_t)pts.size();
    pts.insert(pts.end(), pb.xa.begin(), pb.xa.end());
    X.xbase[1] = X.base_b2 + X.n.b2;
#ifdef ZK_TEST_HOOKS
    X.hook_g1.assign(pts.begin() + X.xbase[2], pts.end());
    X.hook_d.assign(pts.begin() + 2 * (size_t)n_rows, pts.begin() + 2 * (size_t)n_rows + nv);
#endif
    const bool values = merge_values_on();   // (the widths of a run with the switch off stay those of a set without pairs)
    const uint32_t c_set = pick_window(live + P->n_b1 - (values ? std::min<size_t>(X.exp_l + X.exp_b1, live) : 0), 1);
    ZK_TRY(P->g1d.build_with_tail(pts, P->g1, P->off_a, P->g1.n_points - P->off_a, c_set));
    P->g1d_lone.alias(P->g1d, P->g1_lone.c);
    if (X.ready) {
        P->g1da.alias(P->g1d, values ? pick_window(P->n_a - std::min(X.exp_a, P->n_a), 3) : P->g1a.c);
        std::vector<HG2A> pts2(P->n_b2 + 2, HG2A::inf());
        bool ok = P->vk_bytes.size() >= 864;
        for (uint32_t i = 0; ok && i < P->n_b2; i++) ok = zkhost::g2_from_uncompressed(P->enc_b2.data() + (size_t)i * 192, &pts2[i]) == zkhost::DEC_OK;
        ok = ok && zkhost::g2_from_uncompressed(P->vk_bytes.data() + 192, &pts2[P->n_b2]) == zkhost::DEC_OK &&
             zkhost::g2_from_uncompressed(P->vk_bytes.data() + 672, &pts2[P->n_b2 + 1]) == zkhost::DEC_OK;
        if (!ok) return fail(ZK_ERR_IO, "internal: the b_g2 query does not decode a second time");
        pts2.insert(pts2.end(), pb.b2.begin(), pb.b2.end());
        pts2.insert(pts2.end(), pb.xb2.begin(), pb.xb2.end());
#ifdef ZK_TEST_HOOKS
        X.hook_g2.assign(pts2.begin() + X.xbase[1], pts2.end());
#endif
        const uint32_t c2 = values ? pick_window(P->n_b2 - std::min(X.exp_b2, P->n_b2), 2) : P->g2.c;
        ZK_TRY(P->g2p.build(pts2, c2, false, "pair bases (G2)"));
        P->g2p_lone.alias(P->g2p, getenv("ZKAMD_WINDOW_BITS_G2") || c2 <= 10 ? c2 : 10u);
    }
    P->drv.n_rows = n_rows;
    P->drv.off_a = (uint32_t)pts.size();
    P->drv.off_b1 = P->drv.off_a + P->n_a + 2;
    P->drv.circuit = R->id;
    static std::atomic<uint32_t> serial{1};
    P->drv.serial = serial++;
    P->drv.bind_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    P->drv.ready = true;
    if (getenv("ZKAMD_TRACE_HOST"))
        fprintf(stderr, "[zkamd] derived bases: 2 x %u + %u points, %u entries of C, width %u, %.1f ms, table %.2f GB\n", n_rows, nv, nnz,
                c_set, P->drv.bind_ms, (double)P->g1d.bytes / 1e9);
    if (getenv("ZKAMD_TRACE_HOST") && X.ready)
        fprintf(stderr, "[zkamd] value pairs: bases a %u, b_g2 %u, l %u, b_g1 %u; merges expected per proof %u, %u, %u, %u; widths "
                        "C' %u, A %u, G2 %u; G2 table %.2f GB\n", X.n.a, X.n.b2, X.n.l, X.n.b1, X.exp_a, X.exp_b2, X.exp_l, X.exp_b1,
                c_set, P->g1da.c, P->g2p.c, (double)P->g2p.bytes / 1e9);
    if (getenv("ZKAMD_TRACE_HOST") && X.ready)
        for (uint32_t l = 3; l <= zkpairs::RUN_MAX; l++)
            fprintf(stderr, "[zkamd] value runs: bases of %u members: a %u, b_g2 %u, l %u, b_g1 %u\n", l, X.xn[0][l - 3], X.xn[1][l - 3],
                    X.xn[2][l - 3], X.xn[3][l - 3]);
    return ZK_OK;
}

// row evaluations + create_proof of the np assignments in R->z[slot] (Montgomery form)
// derived: the caller is one of the statement-to-proof entries, which take the four-transform form over the derived bases
// of the pair (built here the first time); zk_prove_batch_witness keeps the key's own bases
zk_status prove_from_z(zk_params* P, zk_r1cs* R, size_t np, int slot, const uint8_t* rs, uint8_t* proofs_out, bool derived) {
    const uint32_t nv = R->n_in + R->n_aux, n_rows = R->n_con + R->n_in;
    if (derived) {
        ZK_TRY(ensure_derived(P, R));
        derived = P->drv.ready && P->drv.circuit == R->id;
    }
    ZK_TRY(R->abc.ensure(3 * np * (size_t)n_rows * 32));
    zkdev::R1csMat mm[3];
    for (int m = 0; m < 3; m++)
        mm[m] = zkdev::R1csMat{R->row_ptr[m].as<uint32_t>(), R->col[m].as<uint32_t>(), R->coeff[m].as<uint32_t>()};
    {
        ProfScope ps("r1cs_eval");
        ZK_LAUNCH(zkdev::k_r1cs_eval, dim3((n_rows + 255) / 256, 3, (unsigned)np), dim3(256), 0, g_stream, mm[0], mm[1], mm[2],
                  (const uint32_t*)R->z[slot].as<uint32_t>(), R->abc.as<uint32_t>(), R->n_con, R->n_in, nv, n_rows,
                  np * (size_t)n_rows);
    }
    HIP_TRY(hipGetLastError());
    zk_batch_dev bt;
    bt.n_rows = n_rows;
    bt.n_inputs = R->n_in;
    bt.n_aux = R->n_aux;
    bt.flags = ZK_FR_MONTGOMERY;
    bt.d_a = R->abc.as<uint32_t>();
    bt.d_b = R->abc.as<uint32_t>() + np * (size_t)n_rows * 8;
    bt.d_c = R->abc.as<uint32_t>() + 2 * np * (size_t)n_rows * 8;
    bt.d_wit = R->z[slot].p;
    bt.a_aux_density = R->a_aux_density.data();
    bt.b_input_density = R->b_input_density.data();
    bt.b_aux_density = R->b_aux_density.data();
    return prove_batch_dev(P, np, &bt, rs, proofs_out, derived);
}

zk_status prove_batch_witness(zk_params* P, zk_r1cs* R, size_t n, const uint8_t* witness, uint32_t flags, const uint8_t* rs,
                              uint8_t* proofs_out, bool derived) {
    if (!P || !R || !witness || !rs || !proofs_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    if (R->device != P->device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
    ZK_TRY(use_device(P->device));
    const uint32_t nv = R->n_in + R->n_aux, n_rows = R->n_con + R->n_in;
    if (n_rows > P->m) return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    const size_t chunk = ProveTunables::read().batch_chunk;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        ZK_TRY(R->z[0].ensure(np * (size_t)nv * 32));
        HIP_TRY(hipMemcpyAsync(R->z[0].p, witness + first * (size_t)nv * 32, np * (size_t)nv * 32, hipMemcpyHostToDevice, g_stream));
        ZK_TRY(P->bad.ensure(8));
        HIP_TRY(hipMemsetAsync(P->bad.as<uint32_t>() + 1, 0, 4, g_stream));
        if (!(flags & ZK_FR_MONTGOMERY)) {
            const size_t cnt = np * (size_t)nv;
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, R->z[0].as<uint32_t>(),
                      (const uint32_t*)R->z[0].as<uint32_t>(), 0u, cnt, P->bad.as<uint32_t>() + 1);
        }
        ZK_TRY(prove_from_z(P, R, np, 0, rs + first * 64, proofs_out + first * 192, derived));
        if (P->pin_bad.as<uint32_t>()[1] & zkdev::ZK_BAD_SCALAR)
            return fail(ZK_ERR_INVALID_ARGUMENT, "a witness scalar is not a canonical field element (>= r)");
    }
    return ZK_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// transfer-circuit witness calculator (transfer_witness.h) behind the C ABI
// ------------------------------------------------------------------------------------------
namespace {

zk_status transfer_decode(const zk_transfer_statement& in, size_t index, zkwit::Statement* out) {
    static const uint64_t FS[4] = ZK_JUBJUB_FS_MODULUS_64;
    auto scalar = [&](const uint8_t* b, uint64_t (&v)[4], const char* what) -> zk_status {
        load_scalar_le(b, v);
        for (int i = 3; i >= 0; i--) {
            if (v[i] < FS[i]) return ZK_OK;
            if (v[i] > FS[i]) break;
        }
        return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index) + ": " + what + " is not a canonical Fs scalar");
    };
    auto point = [&](const uint8_t* b, zkwit::JPoint* p, const char* what) -> zk_status {
        if (!zkwit::decode_point(b, p))
            return fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(index) + ": " + what + " is not a Jubjub point");
        return ZK_OK;
    };
    out->amount = in.amount;
    out->remaining_balance = in.remaining_balance;
    out->fee = in.fee;
    ZK_TRY(scalar(in.randomness, out->randomness, "randomness"));
    ZK_TRY(scalar(in.alpha, out->alpha, "alpha"));
    ZK_TRY(scalar(in.dec_key_sender, out->dec_key, "dec_key_sender"));
    ZK_TRY(point(in.proof_generation_key, &out->pgk, "proof_generation_key"));
    ZK_TRY(point(in.enc_key_recipient, &out->enc_key_recipient, "enc_key_recipient"));
    ZK_TRY(point(in.enc_balance_left, &out->enc_balance_left, "enc_balance_left"));
    ZK_TRY(point(in.enc_balance_right, &out->enc_balance_right, "enc_balance_right"));
    ZK_TRY(point(in.g_epoch, &out->g_epoch, "g_epoch"));
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

zk_status anonymous_witness(const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* out) {
    if ((!st || !out) && n) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    static_assert(zkwit::ANON_SIZE == ZK_ANONYMOUS_SIZE, "anonymity set size");
    return witness_batch<zkwit::AnonStatement>(
        n, ZK_ANONYMOUS_N_INPUTS, ZK_ANONYMOUS_N_AUX, flags, out,
        [&](size_t i, zkwit::AnonStatement* s) { return anonymous_decode(st[i], i, s); },
        [](const zkwit::AnonStatement& s, zkwit::Wit& w) { zkwit::synthesize_anonymous(s, w); });
}

}  // namespace

// ------------------------------------------------------------------------------------------
// stand-alone MSM / NTT handles
// ------------------------------------------------------------------------------------------
struct zk_msm {
    int group = 1, device = 0;
    size_t n = 0;
    size_t slice = 0;   // > 0: the multiexp runs as ceil(n / slice) independent jobs (msm_slice below)
    MsmG1 g1;
    MsmG2 g2;
    DevBuf map, scal, conv, sstat;
    bool has_map = false;
    uint32_t vb_window = 0;   // > 0: variable-base mode with this many bits per digit (no doubling table)
};
struct zk_ntt {
    int device = 0;
    NttPlan plan;
};

namespace {

// ZKAMD_MSM_SLICE = k runs a stand-alone multiexp as ceil(n / k) independent jobs over consecutive
// runs of the bases, i.e. as a batch (LDS sort per job, reduction tree over all jobs, slice results
// added on the host).  Off by default: the narrower windows a slice can afford cost more additions
// than the cheaper sort saves - measured on 2^20 G1 points 7.1 ms (k = 4096, c = 13) against 6.0 ms
// as one job with c = 19.  Kept as a tested option (a bucket histogram per slice fits LDS, so it is
// the form to use if the scalars arrive in pieces).
size_t msm_slice(size_t n) {
    if (const char* env = getenv("ZKAMD_MSM_SLICE")) {
        const long v = atol(env);
        return v > 0 && (size_t)v < n ? (size_t)v : 0;
    }
    return 0;
}

// Digits of w bits at fixed positions: W = ceil(255 / w) jobs of 2^(w-1) buckets each.  Minimise, in mixed additions,
//   W * (n + beta * 2^(w-1))      (beta = the cost of reducing one bucket, as in pick_window)
// over the widths whose bucket histogram the sort can hold; a width whose TOP digit is left with only a few bits
// (255 mod w small) sends all n points of that job into a handful of buckets - thousands of task partials merged by a
// few workgroups behind everybody else - so its last job is priced at a full one plus that merge.
uint32_t pick_vb_window(size_t n, int group) {
    double best = 1e300;
    uint32_t w = 2;
    const double beta = group == 2 ? 12.0 : 6.0;
    for (uint32_t k = 2; k <= 20; k++) {
        const uint32_t W = (255 + k - 1) / k, top_bits = 255 - (W - 1) * k;
        double cost = (double)W * ((double)(n ? n : 1) + beta * (double)((size_t)1 << (k - 1)));
        if (top_bits + 4 < k) cost += 0.15 * (double)(n ? n : 1);   // the degenerate top digit (measured: 0.4 ms at 2^20 points)
        if (cost < best) {
            best = cost;
            w = k;
        }
    }
    return w;
}

zk_status msm_configure(zk_msm* M, int group, size_t n, int window_bits, bool variable, uint32_t* c_out) {
    M->group = group;
    M->n = n;
    M->slice = (window_bits > 0 || variable) ? 0 : msm_slice(n);
    M->vb_window = 0;
    // (a stand-alone handle is one or a few jobs: its reduction is the compiled few-jobs path, bucket cost 6 - group 4)
    uint32_t c = window_bits > 0 ? (uint32_t)window_bits : pick_window(M->slice ? M->slice : n, group == 1 ? 4 : group);
    if (variable) {
        const uint32_t w = window_bits > 0 ? (uint32_t)window_bits : pick_vb_window(n, group);
        if (w < 2 || w > 20) return fail(ZK_ERR_INVALID_ARGUMENT, "window_bits out of range [2, 20] for the variable-base mode");
        M->vb_window = w;
        c = w + 1;   // odd magnitudes < 2^w share the kernels' bucket layout for c = w + 1
    }
    if (c < 2 || c > 22) return fail(ZK_ERR_INVALID_ARGUMENT, "window_bits out of range [2, 22]");
    *c_out = c;
    return ZK_OK;
}

zk_status msm_create(int group, const uint8_t* bases, size_t n, int window_bits, int checked, int device, zk_msm** out,
                     bool variable = false) {
    if (group != 1 && group != 2) return fail(ZK_ERR_INVALID_ARGUMENT, "group must be 1 (G1) or 2 (G2)");
    if (!bases && n) return fail(ZK_ERR_INVALID_ARGUMENT, "null bases");
    ZK_TRY(use_device(device));
    zk_msm* M = new (std::nothrow) zk_msm();
    if (!M) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    struct Guard {
        zk_msm* p;
        ~Guard() { delete p; }
    } guard{M};
    M->device = device;
    uint32_t c = 0;
    ZK_TRY(msm_configure(M, group, n, window_bits, variable, &c));
    // the encodings are decoded on the device (msm.h k_decode_uncompressed: 0.1 ms for 2^20 points, the host loop it
    // replaces 0.11 s); points at infinity are legal multiexp bases: they are mapped out (map = -1)
    DevBuf raw;
    uint32_t n_inf = 0;
    if (group == 1) {
        ZK_TRY(M->g1.decode_enqueue(bases, n, c, !variable, raw, M->map, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        ZK_TRY(M->g1.decode_finish("base", &n_inf));
        ZK_TRY(M->g1.finish_build(checked != 0, "bases", !variable));
    } else {
        ZK_TRY(M->g2.decode_enqueue(bases, n, c, !variable, raw, M->map, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        ZK_TRY(M->g2.decode_finish("base", &n_inf));
        ZK_TRY(M->g2.finish_build(checked != 0, "bases", !variable));
    }
    M->has_map = n_inf != 0;
    guard.p = nullptr;
    *out = M;
    return ZK_OK;
}

zk_status msm_run_dev(zk_msm* M, const void* d_scalars, uint32_t flags, uint8_t* out) {
    if (!M || (!d_scalars && M->n) || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(M->device));
    const uint32_t* sc = (const uint32_t*)d_scalars;
    if ((flags & ZK_FR_MONTGOMERY) && M->n) {
        ZK_TRY(M->conv.ensure(M->n * 32));
        ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((M->n + 255) / 256)), dim3(256), 0, g_stream, M->conv.as<uint32_t>(), sc,
                  1u, M->n);
        sc = M->conv.as<uint32_t>();
    }
    // a sliced multiexp is a batch of independent jobs over consecutive runs of the bases (their
    // table entries start at `first`; with a map the map already holds absolute positions)
    std::vector<MsmJob> jobs;
    if (M->vb_window) {
        // one job per digit position, all over the same bases; result = sum_k 2^(w k) R_k
        const uint32_t w = M->vb_window, nd = (255 + w - 1) / w;
        for (uint32_t k = 0; k < nd; k++) {
            MsmJob j = {sc, M->has_map ? M->map.as<int32_t>() : nullptr, (uint32_t)M->n, 0u, (uint32_t)M->n, 0, k + 1, nd};
            jobs.push_back(j);
        }
        auto fold = [&](auto& res, auto zero) {
            auto acc = zero;
            for (size_t k = res.size(); k-- > 0;) {
                for (uint32_t d = 0; d < w; d++) acc = zkhost::pdbl(acc);
                acc = zkhost::padd(acc, res[k]);
            }
            return acc;
        };
        if (M->group == 1) {
            std::vector<HG1> res;
            ZK_TRY(M->g1.run(jobs, res));
            zkhost::g1_to_uncompressed(zkhost::to_affine(fold(res, HG1::inf())), out);
        } else {
            std::vector<HG2> res;
            ZK_TRY(M->g2.run(jobs, res));
            zkhost::g2_to_uncompressed(zkhost::to_affine(fold(res, HG2::inf())), out);
        }
        return ZK_OK;
    }
    const size_t sl = M->slice ? M->slice : M->n;
    for (size_t first = 0; first < M->n; first += sl) {
        const uint32_t cnt = (uint32_t)std::min(sl, M->n - first);
        MsmJob j = {sc + first * 8, M->has_map ? M->map.as<int32_t>() + first : nullptr, cnt,
                    M->has_map ? 0u : (uint32_t)first, (uint32_t)M->n, 0, 0, 0};
        jobs.push_back(j);
    }
    if (M->group == 1) {
        std::vector<HG1> res;
        ZK_TRY(M->g1.run(jobs, res));
        HG1 sum = HG1::inf();
        for (const HG1& r : res) sum = zkhost::padd(sum, r);
        zkhost::g1_to_uncompressed(zkhost::to_affine(sum), out);
    } else {
        std::vector<HG2> res;
        ZK_TRY(M->g2.run(jobs, res));
        HG2 sum = HG2::inf();
        for (const HG2& r : res) sum = zkhost::padd(sum, r);
        zkhost::g2_to_uncompressed(zkhost::to_affine(sum), out);
    }
    return ZK_OK;
}

zk_status check_scalars(const uint8_t* scalars, size_t n, uint32_t flags) {
    if (flags & ZK_FR_MONTGOMERY) return ZK_OK;
    for (size_t i = 0; i < n; i++) {
        uint64_t v[4];
        load_scalar_le(scalars + i * 32, v);
        if (!scalar_lt_r(v)) return fail(ZK_ERR_INVALID_ARGUMENT, "scalar " + std::to_string(i) + " is not < r");
    }
    return ZK_OK;
}

// the caller's plain scalars must be < r (fr.rs:276-289: FrRepr -> Fr fails otherwise); the scalars of a multiexp are
// checked on the device, beside the multiexp
zk_status scalars_check_enqueue(zk_msm* M, const void* d_scalars, uint32_t flags, hipStream_t st) {
    ZK_TRY(M->sstat.ensure(4));
    HIP_TRY(hipMemsetAsync(M->sstat.p, 0xff, 4, st));
    if (!(flags & ZK_FR_MONTGOMERY) && M->n)
        ZK_LAUNCH(zkdev::k_fr_first_noncanonical, dim3((unsigned)((M->n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_scalars,
                  M->n, M->sstat.as<uint32_t>());
    return ZK_OK;
}
zk_status scalars_check_finish(zk_msm* M) {
    uint32_t v = 0xffffffffu;
    HIP_TRY(hipMemcpy(&v, M->sstat.p, 4, hipMemcpyDeviceToHost));
    if (v != 0xffffffffu) return fail(ZK_ERR_INVALID_ARGUMENT, "scalar " + std::to_string(v) + " is not < r");
    return ZK_OK;
}

zk_status msm_run(zk_msm* M, const uint8_t* scalars, uint32_t flags, uint8_t* out) {
    if (!M || (!scalars && M->n) || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(M->device));
    ZK_TRY(M->scal.ensure(M->n * 32 + 32));
    if (M->n) HIP_TRY(hipMemcpyAsync(M->scal.p, scalars, M->n * 32, hipMemcpyHostToDevice, g_stream));
    ZK_TRY(scalars_check_enqueue(M, M->scal.p, flags, g_stream));
    uint8_t res[192];
    ZK_TRY(msm_run_dev(M, M->scal.p, flags, res));   // waits for the stream
    ZK_TRY(scalars_check_finish(M));
    memcpy(out, res, M->group == 1 ? 96 : 192);
    return ZK_OK;
}

// One-shot multiexp over fresh bases (zk_msm_g1 / zk_msm_g2 = bellman's multiexp(FullDensity) called once): variable-base
// Pippenger - no table of doublings is built for bases that are used once - with the encodings decoded on the device and
// ONE wait for the whole call: upload, decode, scalar check, the bucket passes of every digit position, then the verdicts
// and the window sums come back together.  The handle (workspaces, the slice of decoded bases) is kept per (device, group)
// and reused by the next call, so a caller that makes many such calls pays for the allocations once; calls are serialised.
struct OneShotCache {
    std::mutex mu;
    std::map<int, zk_msm*> handles;   // key: device * 4 + group
    std::map<int, DevBuf*> raws;      // the uploaded encodings (never freed: static destructors run after the HIP runtime's)
    DevBuf* raw(int key) {
        DevBuf*& r = raws[key];
        if (!r) r = new DevBuf();
        return r;
    }
};
OneShotCache g_oneshot;

// what the cached handle of a one-shot call keeps at most (decoded bases, pairs, sort and reduction workspaces: ~1.1 KB per
// base): above it the call frees the handle again before it returns - 2^20 bases stay cached (the repeated call of the bench),
// a 2^24-base call does not leave 18 GB behind.  zk_msm_cache_release() drops everything at once.
constexpr size_t ONESHOT_KEEP_BASES = (size_t)1 << 21;

void oneshot_drop(int key) {
    auto it = g_oneshot.handles.find(key);
    if (it != g_oneshot.handles.end()) {
        delete it->second;
        g_oneshot.handles.erase(it);
    }
    auto ir = g_oneshot.raws.find(key);
    if (ir != g_oneshot.raws.end()) ir->second->release();
}

zk_status msm_oneshot(int group, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out) {
    if ((!bases || !scalars) && n) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null output");
    const int dev = g_device >= 0 ? g_device : 0;
    ZK_TRY(use_device(dev));
    std::lock_guard<std::mutex> lock(g_oneshot.mu);
    const int key = dev * 4 + group;
    zk_msm*& M = g_oneshot.handles[key];
    if (!M) {
        M = new (std::nothrow) zk_msm();
        if (!M) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
        M->device = dev;
    }
    // Asynchronous copies out of the CALLER's `bases` / `scalars` are enqueued below: no path may return while one can still
    // be in flight - the guard waits for the stream on every exit, and drops an oversized handle
    struct Drain {
        int key;
        size_t n;
        ~Drain() {
            (void)hipStreamSynchronize(g_stream);
            if (n > ONESHOT_KEEP_BASES) oneshot_drop(key);
        }
    } drain{key, n};
    uint32_t c = 0;
    ZK_TRY(msm_configure(M, group, n, 0, true, &c));
    DevBuf& raw = *g_oneshot.raw(key);
    raw.is_public = true;
    if (group == 1) ZK_TRY(M->g1.decode_enqueue(bases, n, c, false, raw, M->map, g_stream));
    else ZK_TRY(M->g2.decode_enqueue(bases, n, c, false, raw, M->map, g_stream));
    M->has_map = true;   // (whether a base is the point at infinity is not known before the wait: always consult the map)
    ZK_TRY(M->scal.ensure(n * 32 + 32));
    if (n) HIP_TRY(hipMemcpyAsync(M->scal.p, scalars, n * 32, hipMemcpyHostToDevice, g_stream));
    ZK_TRY(scalars_check_enqueue(M, M->scal.p, 0, g_stream));
    uint8_t res[192];
    ZK_TRY(msm_run_dev(M, M->scal.p, 0, res));   // waits for the stream
    uint32_t n_inf = 0;
    if (group == 1) ZK_TRY(M->g1.decode_finish("base", &n_inf));
    else ZK_TRY(M->g2.decode_finish("base", &n_inf));
    ZK_TRY(scalars_check_finish(M));
    memcpy(out, res, group == 1 ? 96 : 192);
    return ZK_OK;
}

zk_status ntt_run_dev(zk_ntt* T, void* d_data, uint32_t batch, uint32_t flags) {
    if (!T || !d_data) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (batch == 0) return ZK_OK;
    ZK_TRY(use_device(T->device));
    NttPlan& pl = T->plan;
    const bool inverse = flags & ZK_NTT_INVERSE, coset = flags & ZK_NTT_COSET;
    const bool in_br = flags & ZK_NTT_IN_BITREV, out_br = flags & ZK_NTT_OUT_BITREV;
    uint32_t* d = (uint32_t*)d_data;
    const size_t n = pl.n, count = (size_t)batch * n;
    const unsigned eb = (unsigned)((count + 255) / 256);
    if (pl.log_n == 0) return ZK_OK;   // size-1 transform is the identity (bellman: exp = 0)
    // coset_fft scales the (natural-order) input by g^i; icoset_fft scales the (natural-order)
    // output by g^-i; plain ifft scales by 1/n.
    const uint32_t* pre = nullptr;
    const uint32_t* post = nullptr;
    if (!inverse && coset) {
        if (in_br) return fail(ZK_ERR_INVALID_ARGUMENT, "coset_fft needs natural-order input");
        pre = pl.coset_fwd.as<uint32_t>();
    }
    if (inverse && coset) {
        if (out_br) return fail(ZK_ERR_INVALID_ARGUMENT, "icoset_fft produces natural-order output");
        post = pl.coset_inv.as<uint32_t>();
    }
    // DIF: natural -> bit-reversed.  DIT: bit-reversed -> natural.
    const bool dif = !in_br;
    bool post_fused = false;
    if (post && !dif) post_fused = true;   // DIT ends in natural order: fuse the scaling
    ZK_TRY(pl.chain(pl.form(batch), d, batch, (uint32_t)n, dif, inverse, pre, post_fused ? post : nullptr));
    const bool have_br = dif;   // order after the chain
    if (have_br != out_br) {
        ZK_TRY(pl.scratch.ensure(count * 32));
        ZK_LAUNCH(zkdev::k_fr_bitrev, dim3(eb), dim3(256), 0, g_stream, pl.scratch.as<uint32_t>(), d, pl.log_n, count);
        HIP_TRY(hipMemcpyAsync(d, pl.scratch.p, count * 32, hipMemcpyDeviceToDevice, g_stream));
    }
    if (inverse) {
        if (coset && !post_fused) {
            ZK_LAUNCH(zkdev::k_fr_scale, dim3(eb), dim3(256), 0, g_stream, d, post, n, count);
        } else if (!coset) {
            ZK_LAUNCH(zkdev::k_fr_scale, dim3(eb), dim3(256), 0, g_stream, d, pl.consts.as<uint32_t>(), (size_t)1, count);
        }
    }
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace

// what the wallet-level entries (wallet.cpp: gen_proof, the Jubjub host side) need of this translation unit
namespace zkrt {
zk_status lib_prove_from_z(zk_params* P, zk_r1cs* R, size_t np, int slot, const uint8_t* rs, uint8_t* proofs_out) {
    return prove_from_z(P, R, np, slot, rs, proofs_out, true);
}
size_t lib_batch_chunk() { return ProveTunables::read().batch_chunk; }
bool lib_witness_on_host(size_t n) { return witness_on_host(n); }
int lib_params_device(const zk_params* P) { return P->device; }
size_t lib_params_domain(const zk_params* P) { return P->m; }
}  // namespace zkrt

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* zk_strerror(zk_status st) {
    switch (st) {
        case ZK_OK: return "ok";
        case ZK_ERR_ASSIGNMENT_MISSING: return "an assignment for a variable could not be computed";
        case ZK_ERR_DIVISION_BY_ZERO: return "division by zero";
        case ZK_ERR_UNSATISFIABLE: return "unsatisfiable constraint system";
        case ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE: return "polynomial degree is too large";
        case ZK_ERR_UNEXPECTED_IDENTITY: return "encountered an identity element in the CRS";
        case ZK_ERR_IO: return "encountered an I/O error";
        case ZK_ERR_MALFORMED_VERIFYING_KEY: return "malformed verifying key";
        case ZK_ERR_UNCONSTRAINED_VARIABLE: return "auxiliary variable was unconstrained";
        case ZK_ERR_INVALID_ARGUMENT: return "invalid argument";
        case ZK_ERR_DEVICE: return "HIP runtime error";
        case ZK_ERR_NO_DEVICE: return "no HIP device";
        case ZK_ERR_OUT_OF_MEMORY: return "out of memory";
    }
    return "unknown status";
}
const char* zk_last_error(void) { return g_err.c_str(); }
void zk_set_host_threads(int n) { g_host_threads = n > 0 ? n : 0; }

zk_status zk_device_count(int* count) try {
    if (!count) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_params_load(const uint8_t* pk_bytes, size_t len, int checked, int device, zk_params** out) try {
    if (!pk_bytes || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return params_load(pk_bytes, len, checked, device, out);
} ZK_ABI_CATCH
zk_status zk_params_get_info(const zk_params* p, zk_params_info* info) try {
    if (!p || !info) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    info->n_ic = p->n_ic;
    info->n_h = p->n_h;
    info->n_l = p->n_l;
    info->n_a = p->n_a;
    info->n_b_g1 = p->n_b1;
    info->n_b_g2 = p->n_b2;
    info->log_domain = p->log_m;
    info->window_bits = p->g1.c;
    info->n_windows = zkdev::MSM_NPOS;
    info->device = (uint32_t)p->device;
    info->device_bytes = p->g1.bytes + p->g2.bytes + p->ntt.bytes;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_windows(const zk_params* p, uint32_t out[4]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = p->g1.c;
    out[1] = p->g1a.c;
    out[2] = p->g1_lone.c;
    out[3] = p->g2.c;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_merged(const zk_params* p, uint32_t out[3]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = p->grp_a.merged();
    out[1] = p->grp_b1.merged();
    out[2] = p->grp_b2.merged();
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_pairs(const zk_params* p, uint32_t out[8]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    const zk_params::Pairs& X = p->prs;
    const uint32_t v[8] = {X.n.a, X.n.b1, X.n.b2, X.n.l, X.exp_a, X.exp_b1, X.exp_b2, X.exp_l};
    for (int i = 0; i < 8; i++) out[i] = p->drv.ready && X.ready ? v[i] : 0u;
    return ZK_OK;
} ZK_ABI_CATCH
void zk_params_free(zk_params* p) { delete p; }
zk_status zk_params_write_vk(const zk_params* p, uint8_t* out, size_t cap, size_t* len) try {
    if (!p || !len) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *len = p->vk_bytes.size();
    if (out) {
        if (cap < p->vk_bytes.size()) return fail(ZK_ERR_INVALID_ARGUMENT, "output buffer too small");
        memcpy(out, p->vk_bytes.data(), p->vk_bytes.size());
    }
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_prove(zk_params* p, const zk_assignment* asg, const uint8_t r[32], const uint8_t s[32], uint8_t proof_out[192]) try {
    if (!r || !s) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    uint8_t rs[64];
    memcpy(rs, r, 32);
    memcpy(rs + 32, s, 32);
    return prove_batch_host(p, 1, asg, rs, proof_out);
} ZK_ABI_CATCH
zk_status zk_prove_batch(zk_params* p, size_t n, const zk_assignment* asgs, const uint8_t* rs, uint8_t* proofs_out) try {
    return prove_batch_host(p, n, asgs, rs, proofs_out);
} ZK_ABI_CATCH
zk_status zk_prove_batch_dev(zk_params* p, size_t n, const zk_batch_dev* batch, const uint8_t* rs, uint8_t* proofs_out) try {
    return prove_batch_dev(p, n, batch, rs, proofs_out);
} ZK_ABI_CATCH

zk_status zk_r1cs_load(uint32_t n_inputs, uint32_t n_aux, uint32_t n_constraints, const zk_csr* a, const zk_csr* b,
                       const zk_csr* c, int device, zk_r1cs** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const zk_csr* mats[3] = {a, b, c};
    return r1cs_load(n_inputs, n_aux, n_constraints, mats, device, out);
} ZK_ABI_CATCH
void zk_r1cs_free(zk_r1cs* r) { delete r; }

// the natively emitted constraint system of the transfer circuit (transfer_r1cs.h), built once per process
static const zkr1cs::System& transfer_system_cached() { return builtin_system(zkpairs::TRANSFER); }
zk_status zk_transfer_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints) try {
    const zkr1cs::System& sys = transfer_system_cached();
    if (hash_out) sys.fingerprint(hash_out);
    if (n_inputs) *n_inputs = sys.n_inputs;
    if (n_aux) *n_aux = sys.n_aux;
    if (n_constraints) *n_constraints = sys.n_constraints;
    return ZK_OK;
} ZK_ABI_CATCH
static zk_status system_load(const zkr1cs::System& sys, int device, zk_r1cs** out) {
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
    return r1cs_load(sys.n_inputs, sys.n_aux, sys.n_constraints, ptrs, device, out);
}
zk_status zk_transfer_r1cs_load(int device, zk_r1cs** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const zkr1cs::System& sys = transfer_system_cached();
    if (sys.n_inputs != ZK_TRANSFER_N_INPUTS || sys.n_aux != ZK_TRANSFER_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "internal: emitted system has the wrong shape");
    return system_load(sys, device, out);
} ZK_ABI_CATCH
// the anonymous-transfer circuit, emitted the same way
static const zkr1cs::System& anonymous_system_cached() { return builtin_system(zkpairs::ANONYMOUS); }
zk_status zk_anonymous_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints) try {
    const zkr1cs::System& sys = anonymous_system_cached();
    if (hash_out) sys.fingerprint(hash_out);
    if (n_inputs) *n_inputs = sys.n_inputs;
    if (n_aux) *n_aux = sys.n_aux;
    if (n_constraints) *n_constraints = sys.n_constraints;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_anonymous_r1cs_load(int device, zk_r1cs** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const zkr1cs::System& sys = anonymous_system_cached();
    if (sys.n_inputs != ZK_ANONYMOUS_N_INPUTS || sys.n_aux != ZK_ANONYMOUS_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "internal: emitted system has the wrong shape");
    return system_load(sys, device, out);
} ZK_ABI_CATCH
zk_status zk_prove_batch_witness(zk_params* p, zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags,
                                 const uint8_t* rs, uint8_t* proofs_out) try {
    return prove_batch_witness(p, circuit, n, witness, flags, rs, proofs_out, false);   // (a caller's witness: the key's own bases)
} ZK_ABI_CATCH
#ifdef ZK_TEST_HOOKS
// Test hook, NOT part of the ABI (absent from libzkamd.so): zk_prove_batch_witness on the route of the statement-to-proof
// entries - the four-transform form over the derived bases of (p, circuit) - for circuits that have no statement form.
// info[0] = whether the pair has a derived set after the call, info[1] = how many of its bases are the identity (mapped out).
zk_status zk_hook_prove_batch_witness_derived(zk_params* p, zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags,
                                              const uint8_t* rs, uint8_t* proofs_out, uint32_t info[2]) try {
    const zk_status rc = prove_batch_witness(p, circuit, n, witness, flags, rs, proofs_out, true);
    if (info && p && circuit) {
        info[0] = p->drv.ready && p->drv.circuit == circuit->id ? 1u : 0u;
        info[1] = (uint32_t)std::count(p->drv.pos.begin(), p->drv.pos.end(), -1);
    }
    return rc;
} ZK_ABI_CATCH
// Test hook: the layout of the derived set (p, circuit) carries, [Lambda | E | D | a | alpha_1 | delta_1 | b_g1 | beta_1].
// info = [has a set, terms of the H block, of the residual block, of the variables, offset of the A query's copy, of the
// b_g1 query's, recoding width of the set], zeros behind info[0] without one.
zk_status zk_hook_derived_layout(zk_params* p, zk_r1cs* circuit, uint32_t info[7]) try {
    if (!p || !circuit || !info) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::fill(info, info + 7, 0u);
    const zk_params::Derived& D = p->drv;
    if (!D.ready || D.circuit != circuit->id) return ZK_OK;
    info[0] = 1;
    info[1] = info[2] = D.n_rows;
    info[3] = (uint32_t)D.pos.size() - 2 * D.n_rows;
    info[4] = D.off_a;
    info[5] = D.off_b1;
    info[6] = p->g1d.c;
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: the plan of a chunk of np proofs (prove_plan.h) under the environment of the call, no GPU involved: out[0 .. 32) =
// the fields of ProvePlan up to the map, the enumerators as numbers; the batch chunk, the host chunk and the trace switch of
// ProveTunables; the fields of CJobLayout in their order
zk_status zk_hook_prove_plan(size_t np, uint32_t n_in, uint32_t n_aux, uint32_t n_rows, size_t m, uint32_t ga, uint32_t gb2, uint32_t gb1,
                             int derived, uint64_t* out, size_t out_words) try {
    if (!out || out_words < 32) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    const ProveTunables tun = ProveTunables::read();
    const ProvePlan p = prove_plan(np, n_in, n_aux, n_rows, m, ga, gb2, gb1, derived != 0, tun);
    const CJobLayout& L = p.layout;
    const uint64_t f[32] = {p.fold_in_msm, p.host_norm, p.g2_lone, p.split, p.one_stream, (uint64_t)p.g1, (uint64_t)p.map,
                            tun.batch_chunk, tun.host_chunk, tun.trace_host,
                            L.n_in, L.n_aux, L.head, L.ga, L.gb2, L.gb1, L.fold, L.derived, L.w_one, L.w_sum_a, L.w_sum_b2, L.wstride,
                            L.aux, L.rz, L.r, L.sz, L.s, L.rs, L.in_tail, L.sum_b1, L.sum_a, L.cstride};
    std::copy(f, f + 32, out);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: zk_hook_prove_plan for a set with value pairs, counts = pairs of the [a, b_g2, l, b_g1] queries: the same 32 words,
// then the pair fields of CJobLayout in their order (11 words and a zero)
zk_status zk_hook_prove_plan_pairs(size_t np, uint32_t n_in, uint32_t n_aux, uint32_t n_rows, size_t m, uint32_t ga, uint32_t gb2,
                                   uint32_t gb1, int derived, const uint32_t counts[4], uint64_t* out, size_t out_words) try {
    if (!out || !counts || out_words < 44) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    PairCounts pc;
    pc.a = counts[0]; pc.b2 = counts[1]; pc.l = counts[2]; pc.b1 = counts[3];
    const ProveTunables tun = ProveTunables::read();
    const ProvePlan p = prove_plan(np, n_in, n_aux, n_rows, m, ga, gb2, gb1, derived != 0, tun, pc);
    const CJobLayout& L = p.layout;
    const uint64_t f[44] = {p.fold_in_msm, p.host_norm, p.g2_lone, p.split, p.one_stream, (uint64_t)p.g1, (uint64_t)p.map,
                            tun.batch_chunk, tun.host_chunk, tun.trace_host,
                            L.n_in, L.n_aux, L.head, L.ga, L.gb2, L.gb1, L.fold, L.derived, L.w_one, L.w_sum_a, L.w_sum_b2, L.wstride,
                            L.aux, L.rz, L.r, L.sz, L.s, L.rs, L.in_tail, L.sum_b1, L.sum_a, L.cstride,
                            L.pa, L.pb2, L.pl, L.pb1, L.w_end, L.w_b2v, L.w_pair_a, L.w_pair_b2, L.pair_l, L.pair_b1, L.pair_a, 0};
    std::copy(f, f + 44, out);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: the chains of a built-in circuit (value_pairs.h; 0 = transfer, 1 = anonymous) under the densities of its natively
// emitted system, out = [pred A | succ A | pred B | succ B | pred L | succ L | A-dense | B-dense], 8 nv words
zk_status zk_hook_pair_chains(int circuit, int32_t* out, size_t cap, uint32_t* nv_out) try {
    if (circuit != 0 && circuit != 1) return fail(ZK_ERR_INVALID_ARGUMENT, "no such circuit");
    const zkr1cs::System& sys = circuit ? anonymous_system_cached() : transfer_system_cached();
    const uint32_t nv = sys.n_inputs + sys.n_aux;
    if (nv_out) *nv_out = nv;
    if (!out) return ZK_OK;
    if (cap < 8 * (size_t)nv) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    std::vector<uint8_t> a_dense(nv, 0), b_dense(nv, 0);
    for (uint32_t i = 0; i < sys.n_inputs; i++) a_dense[i] = 1;
    for (uint32_t v : sys.m[0].col) a_dense[v] = 1;
    for (uint32_t v : sys.m[1].col) b_dense[v] = 1;
    const std::vector<int32_t> c = zkpairs::chains_of(zkpairs::circuit_probes((zkpairs::Circuit)circuit), sys.n_inputs, a_dense, b_dense);
    std::copy(c.begin(), c.end(), out);
    std::copy(a_dense.begin(), a_dense.end(), out + 6 * (size_t)nv);
    std::copy(b_dense.begin(), b_dense.end(), out + 7 * (size_t)nv);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: links -> chains as the library finalizes them (value_pairs.h chains_finalize), pred in place, succ out
zk_status zk_hook_chains_finalize(int32_t* pred, int32_t* succ, uint32_t nv) try {
    if (!pred || !succ) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<int32_t> p(pred, pred + nv);
    for (int32_t& x : p)
        if (x >= (int32_t)nv) x = -1;
    const std::vector<int32_t> s = zkpairs::chains_finalize(p);
    std::copy(p.begin(), p.end(), pred);
    std::copy(s.begin(), s.end(), succ);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: k_build_scalars itself on ONE witness (plain words, n_in + n_aux scalars) under the layout of a derived chunk with
// the given value pairs and groups of equal bases (ngroups = groups of the [a, b_g2, b_g1] queries, groups = [ptr | member
// variables] as k_build_scalars reads them): links = [pred A | succ A | pred B | succ B | pred L | succ L | qa | qb2 |
// ql | qb1] as the kernel reads them (chains as zk_hook_chains_finalize leaves them), counts = the pairs per query [a, b_g2,
// l, b_g1].  wit_out / cvec_out: the two scalar vectors (layout[0] and layout[1] scalars of 32 bytes; the H block has length 0); layout = [wstride, cstride, w_b2v,
// w_pair_a, w_pair_b2, aux, rz, r, sz, s, rs, in_tail, pair_l, pair_b1, pair_a, w_one, w_sum_a, w_sum_b2, sum_b1, sum_a].
// (avail, cap, sel_*, merges: zk_hook_build_scalars_runs below; null / 2 for the rule of pairs alone)
static zk_status hook_build_scalars(uint32_t n_in, uint32_t n_aux, const uint32_t counts[4], const int32_t* links, const uint32_t ngroups[3],
                                    const uint32_t* groups, int fold, const uint8_t* wit, const uint8_t r[32], const uint8_t s[32],
                                    uint8_t* wit_out, size_t wit_cap, uint8_t* cvec_out, size_t cvec_cap, uint32_t layout[20],
                                    const int32_t* avail, uint32_t cap, uint8_t* sel_w_out, uint8_t* sel_c_out, uint64_t* merges) {
    if (!counts || !links || !ngroups || !groups || !wit || !r || !s || !layout || !n_in) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(0));
    const uint32_t nv = n_in + n_aux;
    PairCounts pc;
    pc.a = counts[0]; pc.b2 = counts[1]; pc.l = counts[2]; pc.b1 = counts[3];
    for (size_t k = 0; k < 10 * (size_t)nv; k++) {
        const uint32_t bound = k < 6 * (size_t)nv ? nv : counts[k / nv - 6];
        if (links[k] < -1 || links[k] >= (int32_t)bound) return fail(ZK_ERR_INVALID_ARGUMENT, "link out of range");
    }
    const uint32_t ng = ngroups[0] + ngroups[1] + ngroups[2];
    for (uint32_t g = 0; g < ng; g++)
        if (groups[g] > groups[g + 1]) return fail(ZK_ERR_INVALID_ARGUMENT, "groups are not monotone");
    if (groups[0] != 0) return fail(ZK_ERR_INVALID_ARGUMENT, "groups do not start at 0");
    for (uint32_t k = 0; k < groups[ng]; k++)
        if (groups[ng + 1 + k] >= nv) return fail(ZK_ERR_INVALID_ARGUMENT, "group member out of range");
    const CJobLayout L = cjob_layout(n_in, n_aux, 0, ngroups[0], ngroups[1], ngroups[2], fold != 0, true, pc);
    const uint32_t f[20] = {L.wstride, L.cstride, L.w_b2v, L.w_pair_a, L.w_pair_b2, L.aux, L.rz, L.r, L.sz, L.s, L.rs, L.in_tail,
                            L.pair_l, L.pair_b1, L.pair_a, L.w_one, L.w_sum_a, L.w_sum_b2, L.sum_b1, L.sum_a};
    std::copy(f, f + 20, layout);
    if (!wit_out || !cvec_out) return ZK_OK;
    if (wit_cap < (size_t)L.wstride * 32 || cvec_cap < (size_t)L.cstride * 32) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    DevBuf d_wit, d_tail, d_links, d_grp, d_out, d_cv, d_bad, d_sw, d_sc;
    ZK_TRY(d_wit.ensure((size_t)nv * 32));
    ZK_TRY(d_tail.ensure(96));
    ZK_TRY(d_links.ensure(11 * (size_t)nv * 4));
    if (avail) {
        ZK_TRY(d_sw.ensure((size_t)L.sel_w + 1));
        ZK_TRY(d_sc.ensure((size_t)L.sel_c + 1));
        HIP_TRY(hipMemcpy(d_links.as<int32_t>() + 10 * (size_t)nv, avail, (size_t)nv * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(d_sw.p, 0xff, (size_t)L.sel_w + 1));   // (a byte nobody writes shows)
        HIP_TRY(hipMemset(d_sc.p, 0xff, (size_t)L.sel_c + 1));
    }
    const size_t grp_words = (size_t)ng + 1 + groups[ng];
    ZK_TRY(d_grp.ensure(grp_words * 4));
    ZK_TRY(d_out.ensure((size_t)L.wstride * 32));
    ZK_TRY(d_cv.ensure((size_t)L.cstride * 32));
    ZK_TRY(d_bad.ensure(8));
    uint8_t tail[96] = {1};
    memcpy(tail + 32, r, 32);
    memcpy(tail + 64, s, 32);
    HIP_TRY(hipMemcpy(d_wit.p, wit, (size_t)nv * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_tail.p, tail, 96, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_links.p, links, 10 * (size_t)nv * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_grp.p, groups, grp_words * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_out.p, 0xff, (size_t)L.wstride * 32));   // (a slot nobody writes shows)
    HIP_TRY(hipMemset(d_cv.p, 0xff, (size_t)L.cstride * 32));
    HIP_TRY(hipMemset(d_bad.p, 0, 8));
    ZK_LAUNCH(zkdev::k_build_scalars, dim3((L.w_end + L.gb1 + 255) / 256, 1u), dim3(256), 0, g_stream, d_out.as<uint32_t>(),
              d_cv.as<uint32_t>(), (const uint32_t*)d_wit.as<uint32_t>(), (const uint32_t*)d_tail.as<uint32_t>(), L, 0u, d_bad.as<uint32_t>(),
              (const uint32_t*)d_grp.as<uint32_t>(), (const int32_t*)d_links.as<int32_t>(), avail ? d_sw.as<uint8_t>() : (uint8_t*)nullptr,
              avail ? d_sc.as<uint8_t>() : (uint8_t*)nullptr, cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(wit_out, d_out.p, (size_t)L.wstride * 32, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cvec_out, d_cv.p, (size_t)L.cstride * 32, hipMemcpyDeviceToHost));
    if (avail) {
        if (L.sel_w) HIP_TRY(hipMemcpy(sel_w_out, d_sw.p, L.sel_w, hipMemcpyDeviceToHost));
        if (L.sel_c) HIP_TRY(hipMemcpy(sel_c_out, d_sc.p, L.sel_c, hipMemcpyDeviceToHost));
        // the host's counter on the same values (value_pairs.h count_merges), per query [a, b_g2, l, b_g1]
        std::vector<Fr> z(nv);
        for (uint32_t i = 0; i < nv; i++) memcpy(&z[i], wit + (size_t)i * 32, 32);   // (plain words: only compared)
        const int32_t* q = links + 6 * (size_t)nv;
        for (uint32_t k = 0; k < 4; k++) {
            const int32_t* pred = links + 2 * (size_t)nv * (k == 0 ? 0 : k == 2 ? 2 : 1);
            merges[k] = zkpairs::count_merges(pred, pred + nv, q + k * (size_t)nv, avail, k, z, cap);
        }
    }
    return ZK_OK;
}
zk_status zk_hook_build_scalars(uint32_t n_in, uint32_t n_aux, const uint32_t counts[4], const int32_t* links, const uint32_t ngroups[3],
                                const uint32_t* groups, int fold, const uint8_t* wit, const uint8_t r[32], const uint8_t s[32],
                                uint8_t* wit_out, size_t wit_cap, uint8_t* cvec_out, size_t cvec_cap, uint32_t layout[20]) try {
    return hook_build_scalars(n_in, n_aux, counts, links, ngroups, groups, fold, wit, r, s, wit_out, wit_cap, cvec_out, cvec_cap, layout,
                              nullptr, 2u, nullptr, nullptr, nullptr);
} ZK_ABI_CATCH
// Test hook: the same with terms of up to `cap` members (2 ... value_pairs.h RUN_MAX).  avail: the word per variable that
// follows the q arrays (a byte per query [a, b_g2, l, b_g1], bit l - 1 = the query has the base of the l members that end
// there, l >= 3).  sel_w_out / sel_c_out: the bytes beside the pair slots, counts[0] + counts[1] and counts[2] + counts[3]
// (+ counts[0] with fold) of them; merges: value_pairs.h count_merges on the same values, per query [a, b_g2, l, b_g1].
zk_status zk_hook_build_scalars_runs(uint32_t n_in, uint32_t n_aux, const uint32_t counts[4], const int32_t* links, const int32_t* avail,
                                     uint32_t cap, const uint32_t ngroups[3], const uint32_t* groups, int fold, const uint8_t* wit,
                                     const uint8_t r[32], const uint8_t s[32], uint8_t* wit_out, size_t wit_cap, uint8_t* cvec_out,
                                     size_t cvec_cap, uint8_t* sel_w_out, uint8_t* sel_c_out, uint64_t merges[4], uint32_t layout[20]) try {
    if (!avail || !sel_w_out || !sel_c_out || !merges) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (cap < 2 || cap > zkpairs::RUN_MAX) return fail(ZK_ERR_INVALID_ARGUMENT, "the cap is not in 2 ... RUN_MAX");
    return hook_build_scalars(n_in, n_aux, counts, links, ngroups, groups, fold, wit, r, s, wit_out, wit_cap, cvec_out, cvec_cap, layout,
                              avail, cap, sel_w_out, sel_c_out, merges);
} ZK_ABI_CATCH
// Test hook: the largest cap the library was built for (value_pairs.h RUN_MAX)
uint32_t zk_hook_run_max(void) { return zkpairs::RUN_MAX; }
// Test hook: the longer bases of the (key, circuit) pair as ensure_derived bound them.  info = [RUN_MAX, nv, pairs a, b_g2, l,
// b_g1, xbase a, b_g2, l, b_g1, points in g1, in g2]; with the outputs given: links (11 nv words, as k_build_scalars reads
// them), alt ([a | b_g2 | l | b_g1], (RUN_MAX - 2) words per pair slot, places among the query's longer bases), g1 / g2 (the
// uncompressed points the tables got from xbase l / xbase b_g2 on), d (nv uncompressed points: the D block of the derived set)
zk_status zk_hook_value_runs(const zk_params* p, uint32_t info[12], int32_t* links, int32_t* alt, uint8_t* g1, uint8_t* g2, uint8_t* d) try {
    if (!p || !info) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    const zk_params::Pairs& X = p->prs;
    if (!p->drv.ready || !X.ready) return fail(ZK_ERR_INVALID_ARGUMENT, "the key has no value pairs");
    const uint32_t nv = (uint32_t)(X.links.size() / 11);
    const uint32_t f[12] = {zkpairs::RUN_MAX, nv, X.n.a, X.n.b2, X.n.l, X.n.b1, X.xbase[0], X.xbase[1], X.xbase[2], X.xbase[3],
                            (uint32_t)X.hook_g1.size(), (uint32_t)X.hook_g2.size()};
    std::copy(f, f + 12, info);
    if (!links) return ZK_OK;
    if (!alt || !g1 || !g2 || !d) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::copy(X.links.begin(), X.links.end(), links);
    for (int k = 0; k < 4; k++) alt = std::copy(X.alt[k].begin(), X.alt[k].end(), alt);
    for (size_t i = 0; i < X.hook_g1.size(); i++) zkhost::g1_to_uncompressed(X.hook_g1[i], g1 + i * 96);
    for (size_t i = 0; i < X.hook_g2.size(); i++) zkhost::g2_to_uncompressed(X.hook_g2[i], g2 + i * 192);
    for (size_t i = 0; i < X.hook_d.size(); i++) zkhost::g1_to_uncompressed(X.hook_d[i], d + i * 96);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: n_jobs multiexp jobs over the bases of a G1 handle, each of n scalars (plain words) through one map, with the
// bytes and alternates of msm.h MsmSelRange over the slots [sel_first, sel_first + sel_n) (sel: sel_n bytes per job, or
// null: jobs without them); out: n_jobs uncompressed points
zk_status zk_hook_msm_select(zk_msm* M, uint32_t n_jobs, uint32_t n, const uint8_t* scalars, const int32_t* map, const uint8_t* sel,
                             const int32_t* alt, uint32_t sel_first, uint32_t sel_n, uint32_t alt_w, uint8_t* out) try {
    if (!M || M->group != 1 || M->vb_window || M->slice || !scalars || !map || !out || !n || !n_jobs)
        return fail(ZK_ERR_INVALID_ARGUMENT, "null argument or not a plain G1 handle");
    if (sel && (!alt || (size_t)sel_first + sel_n > n || alt_w > 6)) return fail(ZK_ERR_INVALID_ARGUMENT, "the bytes do not fit the job");
    for (uint32_t i = 0; i < n; i++)
        if (map[i] < -1 || map[i] >= (int32_t)M->n) return fail(ZK_ERR_INVALID_ARGUMENT, "map out of range");
    for (size_t i = 0; sel && i < (size_t)sel_n * alt_w; i++)
        if (alt[i] < -1 || alt[i] >= (int32_t)M->n) return fail(ZK_ERR_INVALID_ARGUMENT, "alternate out of range");
    ZK_TRY(use_device(M->device));
    DevBuf d_sc, d_map, d_sel, d_alt;
    ZK_TRY(d_sc.ensure((size_t)n_jobs * n * 32));
    ZK_TRY(d_map.ensure((size_t)n * 4));
    HIP_TRY(hipMemcpy(d_sc.p, scalars, (size_t)n_jobs * n * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_map.p, map, (size_t)n * 4, hipMemcpyHostToDevice));
    if (sel) {
        ZK_TRY(d_sel.ensure((size_t)n_jobs * sel_n + 1));
        ZK_TRY(d_alt.ensure((size_t)sel_n * alt_w * 4 + 4));
        HIP_TRY(hipMemcpy(d_sel.p, sel, (size_t)n_jobs * sel_n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_alt.p, alt, (size_t)sel_n * alt_w * 4, hipMemcpyHostToDevice));
    }
    std::vector<MsmJob> jobs;
    for (uint32_t p = 0; p < n_jobs; p++) {
        MsmJob j = {d_sc.as<uint32_t>() + (size_t)p * n * 8, d_map.as<int32_t>(), n, 0u, (uint32_t)M->n, 0, 0, 0};
        jobs.push_back(j);
    }
    zkdev::MsmSelSet sels = {};
    if (sel) sels.r[0] = {d_sel.as<uint8_t>(), d_alt.as<int32_t>(), 0u, n_jobs, sel_n, sel_first, sel_n, alt_w};
    std::vector<HG1> res;
    ZK_TRY(M->g1.run(jobs, res, &sels));
    for (uint32_t p = 0; p < n_jobs; p++) zkhost::g1_to_uncompressed(zkhost::to_affine(res[p]), out + (size_t)p * 96);
    return ZK_OK;
} ZK_ABI_CATCH
#endif

zk_status zk_transfer_witness(const zk_transfer_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    return transfer_witness(st, n, flags, witness_out);
} ZK_ABI_CATCH
zk_status zk_anonymous_witness(const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    return anonymous_witness(st, n, flags, witness_out);
} ZK_ABI_CATCH
zk_status zk_transfer_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_transfer_statement* st,
                                  const uint8_t* rs, uint8_t* proofs_out) try {
    if (!p || !circuit || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (circuit->n_in != ZK_TRANSFER_N_INPUTS || circuit->n_aux != ZK_TRANSFER_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "the loaded constraint matrices are not the transfer circuit's");
    if (circuit->device != p->device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
    if (n == 0) return ZK_OK;
    const size_t nv = ZK_TRANSFER_N_INPUTS + ZK_TRANSFER_N_AUX;
    const size_t chunk = ProveTunables::read().batch_chunk;
    zk_status rc = use_device(p->device);
    if (rc != ZK_OK) return rc;
    if ((size_t)circuit->n_con + circuit->n_in > p->m)
        return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    if (!witness_on_host(n)) {
        // witnesses on the GPU (witness_gpu.h), on the side stream of the copy engine: the kernels of chunk k + 1
        // are latency-bound chains for a few hundred waves and run beside the multiexps of chunk k
        int slot = 0;
        ZK_TRY(witness_gpu_enqueue(circuit, st, std::min(chunk, n), slot, g_copy_stream));
        for (size_t first = 0; first < n; first += chunk) {
            const size_t np = std::min(chunk, n - first), next = first + chunk;
            ZK_TRY(witness_gpu_finish(circuit, np, slot, first));
            if (next < n) ZK_TRY(witness_gpu_enqueue(circuit, st + next, std::min(chunk, n - next), slot ^ 1, g_copy_stream));
            ZK_TRY(prove_from_z(p, circuit, np, slot, rs + first * 64, proofs_out + first * 192, true));
            slot ^= 1;
        }
        return ZK_OK;
    }
    // a handful of statements, or ZKAMD_WITNESS=host: the host calculator (transfer_witness.h) on the host cores; two pinned
    // buffers, the witnesses of chunk k + 1 are computed while the GPU proves chunk k
    const size_t cap = std::min(chunk, n) * nv * 32;
    rc = circuit->host_ensure(2 * cap);
    if (rc != ZK_OK) return rc;
    uint8_t* buf[2] = {(uint8_t*)circuit->host_z, (uint8_t*)circuit->host_z + cap};
    rc = transfer_witness(st, std::min(chunk, n), ZK_FR_MONTGOMERY, buf[0]);
    if (rc != ZK_OK) return rc;
    int cur = 0;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        const size_t next = first + chunk;
        zk_status next_rc = ZK_OK;
        std::string next_err;
        SideThread producer;
        if (next < n)
            producer.start([&, next] {
                next_rc = transfer_witness(st + next, std::min(chunk, n - next), ZK_FR_MONTGOMERY, buf[cur ^ 1], next);
                if (next_rc != ZK_OK) next_err = g_err;   // g_err is thread-local
            });
        rc = prove_batch_witness(p, circuit, np, buf[cur], ZK_FR_MONTGOMERY, rs + first * 64, proofs_out + first * 192, true);
        producer.join();
        if (rc != ZK_OK) return rc;
        if (next_rc != ZK_OK) return fail(next_rc, next_err);
        cur ^= 1;
    }
    return ZK_OK;
} ZK_ABI_CATCH

// Statement -> proof for the anonymous-transfer circuit (core/proofs/src/anonymous.rs:165: create_random_proof of
// AnonymousTransfer): witness generation on the GPU (witness_anon_gpu.h, round 4), the kernels of chunk k + 1 beside the
// proving of chunk k; ZKAMD_WITNESS=host keeps the native host calculator (transfer_witness.h: synthesize_anonymous) on
// the host cores.  Both paths prove every chunk before the first malformed statement's and report that statement in the
// same words.
zk_status zk_anonymous_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_anonymous_statement* st, const uint8_t* rs,
                                   uint8_t* proofs_out) try {
    if (!p || !circuit || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (circuit->n_in != ZK_ANONYMOUS_N_INPUTS || circuit->n_aux != ZK_ANONYMOUS_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "the loaded constraint matrices are not the anonymous-transfer circuit's");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(p->device));
    const size_t nv = ZK_ANONYMOUS_N_INPUTS + ZK_ANONYMOUS_N_AUX;
    size_t chunk = ProveTunables::read().batch_chunk;
    if (chunk > 512) chunk = 512;   // domain 2^16: half the proofs of a transfer chunk fill the same workspaces
    if (!witness_on_host(n)) {
        // witness generation on the GPU (witness_anon_gpu.h), statement in: 1.7 KB instead of 1.6 MB of witness vector; the
        // kernels of chunk k + 1 run beside the multiexps of chunk k (as zk_transfer_prove_batch)
        if (circuit->device != p->device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
        int slot = 0;
        zk_status rc = witness_anon_gpu_enqueue(circuit, st, std::min(chunk, n), slot, g_copy_stream);
        for (size_t first = 0; first < n && rc == ZK_OK; first += chunk) {
            const size_t np = std::min(chunk, n - first), next = first + chunk;
            rc = witness_anon_gpu_finish(circuit, np, slot, first);
            if (rc == ZK_OK && next < n) rc = witness_anon_gpu_enqueue(circuit, st + next, std::min(chunk, n - next), slot ^ 1, g_copy_stream, next);
            if (rc == ZK_OK) rc = prove_from_z(p, circuit, np, slot, rs + first * 64, proofs_out + first * 192, true);
            slot ^= 1;
        }
        if (rc != ZK_OK) {
            const std::string why = g_err;
            (void)hipStreamSynchronize(g_copy_stream);   // no witness kernel of a later chunk stays in flight behind an error
            g_err = why;
        }
        return rc;
    }
    const size_t cap = std::min(chunk, n) * nv * 32;
    ZK_TRY(circuit->host_ensure(2 * cap));
    uint8_t* buf[2] = {(uint8_t*)circuit->host_z, (uint8_t*)circuit->host_z + cap};
    auto witness = [&](size_t first, size_t np, uint8_t* out) -> zk_status {
        return witness_batch<zkwit::AnonStatement>(
            np, ZK_ANONYMOUS_N_INPUTS, ZK_ANONYMOUS_N_AUX, ZK_FR_MONTGOMERY, out,
            [&](size_t i, zkwit::AnonStatement* s) { return anonymous_decode(st[first + i], first + i, s); },
            [](const zkwit::AnonStatement& s, zkwit::Wit& w) { zkwit::synthesize_anonymous(s, w); });
    };
    ZK_TRY(witness(0, std::min(chunk, n), buf[0]));
    int cur = 0;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first), next = first + chunk;
        zk_status next_rc = ZK_OK;
        std::string next_err;
        SideThread producer;
        if (next < n)
            producer.start([&, next] {
                next_rc = witness(next, std::min(chunk, n - next), buf[cur ^ 1]);
                if (next_rc != ZK_OK) next_err = g_err;
            });
        // prove_batch_witness cuts at its own chunk size: keep the two equal for this call
        zk_status rc = ZK_OK;
        for (size_t off = 0; off < np && rc == ZK_OK; off += chunk)
            rc = prove_batch_witness(p, circuit, std::min(chunk, np - off), buf[cur] + off * nv * 32, ZK_FR_MONTGOMERY,
                                     rs + (first + off) * 64, proofs_out + (first + off) * 192, true);
        producer.join();
        if (rc != ZK_OK) return rc;
        if (next_rc != ZK_OK) return fail(next_rc, next_err);
        cur ^= 1;
    }
    return ZK_OK;
} ZK_ABI_CATCH

// The witness vectors the GPU generator of the anonymous circuit produces, copied back to the host (tests: element by
// element against zk_anonymous_witness).  witness_out: n x (105 + 50429) x 32 bytes.
zk_status zk_anonymous_witness_gpu(zk_r1cs* circuit, const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    if (!circuit || (n && (!st || !witness_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (circuit->n_in != ZK_ANONYMOUS_N_INPUTS || circuit->n_aux != ZK_ANONYMOUS_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "the loaded constraint matrices are not the anonymous-transfer circuit's");
    ZK_TRY(use_device(circuit->device));
    const size_t nv = ZK_ANONYMOUS_N_INPUTS + ZK_ANONYMOUS_N_AUX, chunk = 256;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        ZK_TRY(witness_anon_gpu_enqueue(circuit, st + first, np, 0, g_stream, first));
        ZK_TRY(witness_anon_gpu_finish(circuit, np, 0, first));
        if (!(flags & ZK_FR_MONTGOMERY)) {
            const size_t cnt = np * nv;
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, circuit->z[0].as<uint32_t>(),
                      (const uint32_t*)circuit->z[0].as<uint32_t>(), 1u, cnt, (uint32_t*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipMemcpy(witness_out + first * nv * 32, circuit->z[0].p, np * nv * 32, hipMemcpyDeviceToHost));
    }
    return ZK_OK;
} ZK_ABI_CATCH

// The witness vectors the GPU generator produces, copied back to the host: lets the tests compare it with the
// host calculator (zk_transfer_witness) element by element.  witness_out: n x (23 + 19955) x 32 bytes.
zk_status zk_transfer_witness_gpu(zk_r1cs* circuit, const zk_transfer_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    if (!circuit || (n && (!st || !witness_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (circuit->n_in != ZK_TRANSFER_N_INPUTS || circuit->n_aux != ZK_TRANSFER_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "the loaded constraint matrices are not the transfer circuit's");
    ZK_TRY(use_device(circuit->device));
    const size_t nv = ZK_TRANSFER_N_INPUTS + ZK_TRANSFER_N_AUX, chunk = ProveTunables::read().batch_chunk;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        ZK_TRY(witness_gpu_enqueue(circuit, st + first, np, 0, g_stream));
        ZK_TRY(witness_gpu_finish(circuit, np, 0, first));
        if (!(flags & ZK_FR_MONTGOMERY)) {
            const size_t cnt = np * nv;
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, circuit->z[0].as<uint32_t>(),
                      (const uint32_t*)circuit->z[0].as<uint32_t>(), 1u, cnt, (uint32_t*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(g_stream));
        HIP_TRY(hipMemcpy(witness_out + first * nv * 32, circuit->z[0].p, np * nv * 32, hipMemcpyDeviceToHost));
    }
    return ZK_OK;
} ZK_ABI_CATCH

// ------------------------------------------------------------------------------------------
// zk_pipeline: a stream of statement batches.  zk_transfer_prove_batch overlaps the witnesses of
// chunk k + 1 with the GPU work of chunk k INSIDE one call; a service that proves batch after batch
// wants the same overlap ACROSS calls.  submit() queues a batch and returns; a producer thread computes
// its witnesses (host cores) into one of two page-locked buffers while the GPU thread proves the batch
// before it; wait() returns when everything submitted so far is proved.
// ------------------------------------------------------------------------------------------
}  // extern "C"

struct zk_pipeline {
    struct Job {
        const zk_transfer_statement* st;
        const uint8_t* rs;
        uint8_t* out;
        size_t n, index_base;
        int slot;
    };
    zk_params* P = nullptr;
    zk_r1cs* R = nullptr;
    // lanes 1 .. (ZKAMD_PIPELINE_LANES, default 2): further workers with their own workspaces and streams over the
    // same tables - several chunks in flight, the sort / reduction / fold / witness phases of one beside the
    // accumulation of another
    static constexpr int MAX_LANES = 4;
    zk_params* Pl[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    zk_r1cs* Rl[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    std::thread t_lane[MAX_LANES];
    int n_lanes = 1;      // lanes started at create
    int live_lanes = 1;   // ... minus the ones that retired when their workspaces did not fit (mu held)
    size_t chunk = 0, nv = 0;   // (proofs per launch set: ProveTunables, at zk_pipeline_create)
    PinBuf buf[2];
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> q_wit, q_gpu;
    bool slot_free[2] = {true, true};
    size_t in_flight = 0;
    zk_status err = ZK_OK;
    std::string err_msg;
    bool stop = false;
    std::thread t_wit, t_gpu;

    void fail_with(zk_status st, const std::string& msg) {   // mu held
        if (err == ZK_OK) {
            err = st;
            err_msg = msg;
        }
    }
    void run_wit() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || (!q_wit.empty() && (slot_free[0] || slot_free[1])); });
                if (stop) return;
                j = q_wit.front();
                q_wit.pop_front();
                j.slot = slot_free[0] ? 0 : 1;
                slot_free[j.slot] = false;
                if (err != ZK_OK) {   // a failed stream drains without doing work
                    q_gpu.push_back(j);
                    cv.notify_all();
                    continue;
                }
            }
            zk_status rc = guarded([&] { return transfer_witness(j.st, j.n, ZK_FR_MONTGOMERY, buf[j.slot].as<uint8_t>(), j.index_base); });
            std::lock_guard<std::mutex> lk(mu);
            if (rc != ZK_OK) fail_with(rc, g_err);
            q_gpu.push_back(j);
            cv.notify_all();
        }
    }
    // GPU-witness mode: one thread.  The witness kernels of the job behind the current one are enqueued (side
    // stream, other assignment buffer) before the current job is proved, so they run beside its multiexps.
    void run_gpu_witness(int lane) {
        Job cur{}, nxt{};
        bool have_cur = false;
        int slot = 0;
        g_lane = lane;
        zk_params* Pw = lane ? Pl[lane] : P;   // this lane's handles: its own workspaces over the shared tables
        zk_r1cs* Rw = lane ? Rl[lane] : R;
        if (use_device(Pw->device) != ZK_OK) {
            // no context on this lane (stream creation / out of memory): report it and keep DRAINING the queue, so
            // that wait() and free() never block on jobs nobody will take
            std::unique_lock<std::mutex> lk(mu);
            fail_with(ZK_ERR_DEVICE, g_err);
            for (;;) {
                cv.wait(lk, [&] { return stop || !q_wit.empty(); });
                if (stop) return;
                q_wit.pop_front();
                in_flight--;
                cv.notify_all();
            }
        }
        const hipStream_t wstream = g_copy_stream;
        auto start = [&](Job& j, int s) -> zk_status {
            j.slot = s;
            return guarded([&] { return witness_gpu_enqueue(Rw, j.st, j.n, s, wstream); });
        };
        for (;;) {
            zk_status rc = ZK_OK;
            if (!have_cur) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q_wit.empty(); });
                if (stop) return;
                cur = q_wit.front();
                q_wit.pop_front();
                const bool skip = err != ZK_OK;
                lk.unlock();
                cur.slot = slot;
                if (!skip) rc = start(cur, slot);
                // test hook: a lane beyond the first behaves as if its workspaces did not fit (tests/test_gpu_parity.py)
                if (!skip && lane > 0 && hook_env("ZKAMD_INJECT_LANE_OOM")) rc = fail(ZK_ERR_OUT_OF_MEMORY, "injected: lane workspaces do not fit");
            }
            bool have_nxt = false;
            {
                // (with several lanes a job is only taken ahead of time if the other lanes still find one each)
                std::lock_guard<std::mutex> lk(mu);
                if (q_wit.size() >= (size_t)live_lanes) {
                    nxt = q_wit.front();
                    q_wit.pop_front();
                    have_nxt = true;
                }
            }
            bool skip;
            {
                std::lock_guard<std::mutex> lk(mu);
                skip = err != ZK_OK;
            }
            zk_status rc_next = ZK_OK;
            if (have_nxt && !skip && rc == ZK_OK) rc_next = start(nxt, cur.slot ^ 1);
            if (!skip && rc == ZK_OK) rc = guarded([&] { return witness_gpu_finish(Rw, cur.n, cur.slot, cur.index_base); });
            if (!skip && rc == ZK_OK) rc = guarded([&] { return prove_from_z(Pw, Rw, cur.n, cur.slot, cur.rs, cur.out, true); });
            // nothing of a failed job stays in flight when wait() returns: drain the device BEFORE the job is counted done
            if (rc != ZK_OK || rc_next != ZK_OK) (void)hipDeviceSynchronize();
            if (lane > 0 && (rc == ZK_ERR_OUT_OF_MEMORY || rc_next == ZK_ERR_OUT_OF_MEMORY)) {
                // The workspaces of a lane are allocated when it proves its first chunk; the free-memory estimate at
                // create is only a hint (two ranks on one GPU see the same free bytes - ADVICE r3).  A lane beyond the
                // first that does not get its memory hands its jobs back, releases what it holds and retires: the
                // pipeline degrades to fewer lanes instead of failing in the middle of a batch.
                std::unique_lock<std::mutex> lk(mu);
                if (have_nxt) q_wit.push_front(nxt);
                // (only the job that did NOT get proved goes back: when starting the NEXT job is what ran out of memory, the
                //  current one is finished and counted - ADVICE r4)
                if (rc == ZK_OK && !skip) in_flight--;
                else q_wit.push_front(cur);
                live_lanes--;
                zk_params* mine = Pl[lane];
                zk_r1cs* mine_r = Rl[lane];
                Pl[lane] = nullptr;
                Rl[lane] = nullptr;
                lk.unlock();
                delete mine;      // borrowed tables stay with the original, the lane's own buffers are freed
                delete mine_r;
                std::lock_guard<std::mutex> lk2(mu);
                cv.notify_all();
                return;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc != ZK_OK) fail_with(rc, g_err);
                else if (rc_next != ZK_OK) fail_with(rc_next, g_err);
                in_flight--;
                cv.notify_all();
            }
            if (have_nxt) {
                nxt.slot = cur.slot ^ 1;
                cur = nxt;
                have_cur = true;
                slot = cur.slot;
            } else {
                have_cur = false;
                slot = cur.slot ^ 1;
            }
        }
    }
    void run_gpu() {
        for (;;) {
            Job j;
            bool skip;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q_gpu.empty(); });
                if (stop) return;
                j = q_gpu.front();
                q_gpu.pop_front();
                skip = err != ZK_OK;
            }
            zk_status rc = ZK_OK;
            if (!skip) rc = guarded([&] { return prove_batch_witness(P, R, j.n, buf[j.slot].as<uint8_t>(), ZK_FR_MONTGOMERY, j.rs, j.out, true); });
            std::lock_guard<std::mutex> lk(mu);
            if (rc != ZK_OK) fail_with(rc, g_err);
            slot_free[j.slot] = true;
            in_flight--;
            cv.notify_all();
        }
    }
};

extern "C" {

zk_status zk_pipeline_create(zk_params* p, zk_r1cs* circuit, zk_pipeline** out) try {
    if (!p || !circuit || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (circuit->n_in != ZK_TRANSFER_N_INPUTS || circuit->n_aux != ZK_TRANSFER_N_AUX)
        return fail(ZK_ERR_INVALID_ARGUMENT, "the loaded constraint matrices are not the transfer circuit's");
    if (circuit->device != p->device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
    ZK_TRY(use_device(p->device));
    zk_pipeline* L = new (std::nothrow) zk_pipeline();
    if (!L) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    L->P = p;
    L->R = circuit;
    L->nv = ZK_TRANSFER_N_INPUTS + ZK_TRANSFER_N_AUX;
    L->chunk = ProveTunables::read().batch_chunk;
    if ((size_t)circuit->n_con + circuit->n_in > p->m) {
        delete L;
        return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    }
    (void)zkwit::tables();
    {
        // the derived bases of the pair before the lanes borrow the key's tables: every lane binds to the same set
        const zk_status rc = ensure_derived(p, circuit);
        if (rc != ZK_OK) {
            delete L;
            return rc;
        }
    }
    if (!witness_on_host()) {
        int lanes = 2;
        if (const char* env = getenv("ZKAMD_PIPELINE_LANES")) lanes = atoi(env);
#ifdef ZK_EMU
        lanes = 1;   // the test-only emulation runs one launch at a time
#endif
        if (lanes > zk_pipeline::MAX_LANES) lanes = zk_pipeline::MAX_LANES;
        // Every lane allocates its chunk workspaces the first time it proves (~36 MB per proof of a transfer-circuit chunk:
        // 35 GB at 1024).  The free memory seen here only caps the number of lanes STARTED (a hint: it is check-then-
        // allocate, and another process may take the memory in between); it never refuses the pipeline - lane 0 lets the
        // real allocation report OutOfMemory, and a further lane whose allocation fails later hands its jobs back and
        // retires (run_gpu_witness).  A zk_params that has proved before already holds lane 0's workspaces.
#ifndef ZK_EMU
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                size_t per_lane = L->chunk * ((size_t)36 << 20);
                if (const char* env = getenv("ZKAMD_LANE_BYTES"))
                    if (atoll(env) > 0) per_lane = (size_t)atoll(env);
                const size_t reserve = (size_t)2 << 30;
                const size_t avail = free_b > reserve ? free_b - reserve : 0;
                const size_t lane0 = p->abc.p ? 0 : per_lane;       // nothing more to allocate once it has proved a chunk
                const size_t fit = 1 + (avail > lane0 ? (avail - lane0) / per_lane : 0);
                if ((size_t)lanes > fit) lanes = (int)fit;
            }
        }
#endif
        if (lanes < 1) lanes = 1;
        for (int l = 1; l < lanes; l++) {
            L->Pl[l] = params_clone_for_lane(p);
            L->Rl[l] = r1cs_clone_for_lane(circuit);
            if (!L->Pl[l] || !L->Rl[l]) {   // no room for another set of workspaces: run with the lanes there are
                delete L->Pl[l];
                delete L->Rl[l];
                L->Pl[l] = nullptr;
                L->Rl[l] = nullptr;
                break;
            }
            L->n_lanes = l + 1;
        }
        L->live_lanes = L->n_lanes;
        try {
            L->t_gpu = std::thread([L] { L->run_gpu_witness(0); });
            for (int l = 1; l < L->n_lanes; l++) L->t_lane[l] = std::thread([L, l] { L->run_gpu_witness(l); });
        } catch (const std::system_error& e) {
            zk_pipeline_free(L);
            return fail(ZK_ERR_OUT_OF_MEMORY, std::string("cannot start a pipeline worker: ") + e.what());
        }
    } else {
        for (int k = 0; k < 2; k++) {
            zk_status rc = L->buf[k].ensure(L->chunk * L->nv * 32);
            if (rc != ZK_OK) {
                delete L;
                return rc;
            }
        }
        try {
            L->t_wit = std::thread([L] { L->run_wit(); });
            L->t_gpu = std::thread([L] { L->run_gpu(); });
        } catch (const std::system_error& e) {
            zk_pipeline_free(L);
            return fail(ZK_ERR_OUT_OF_MEMORY, std::string("cannot start a pipeline worker: ") + e.what());
        }
    }
    *out = L;
    return ZK_OK;
} ZK_ABI_CATCH

int zk_pipeline_lanes(const zk_pipeline* L) {
    if (!L) return 0;
    std::lock_guard<std::mutex> lk(const_cast<zk_pipeline*>(L)->mu);
    return L->live_lanes;
}

zk_status zk_pipeline_submit(zk_pipeline* L, size_t n, const zk_transfer_statement* st, const uint8_t* rs, uint8_t* proofs_out) try {
    if (!L || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(L->mu);
    for (size_t first = 0; first < n; first += L->chunk) {
        const size_t np = std::min(L->chunk, n - first);
        L->q_wit.push_back(zk_pipeline::Job{st + first, rs + first * 64, proofs_out + first * 192, np, first, -1});
        L->in_flight++;
    }
    L->cv.notify_all();
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_pipeline_wait(zk_pipeline* L) try {
    if (!L) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_lock<std::mutex> lk(L->mu);
    L->cv.wait(lk, [&] { return L->in_flight == 0; });
    const zk_status rc = L->err;
    if (rc != ZK_OK) g_err = L->err_msg;
    L->err = ZK_OK;   // the stream is usable again after the failure has been reported
    L->err_msg.clear();
    return rc;
} ZK_ABI_CATCH

void zk_pipeline_free(zk_pipeline* L) {
    if (!L) return;
    {
        std::unique_lock<std::mutex> lk(L->mu);
        L->cv.wait(lk, [&] { return L->in_flight == 0; });
        L->stop = true;
        L->cv.notify_all();
    }
    if (L->t_wit.joinable()) L->t_wit.join();
    if (L->t_gpu.joinable()) L->t_gpu.join();
    for (int l = 1; l < zk_pipeline::MAX_LANES; l++) {
        if (L->t_lane[l].joinable()) L->t_lane[l].join();
        delete L->Pl[l];
        delete L->Rl[l];
    }
    delete L;
}

zk_status zk_msm_create(int group, const uint8_t* bases, size_t n, int window_bits, int checked, int device, zk_msm** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return msm_create(group, bases, n, window_bits, checked, device, out);
} ZK_ABI_CATCH
zk_status zk_msm_create_variable(int group, const uint8_t* bases, size_t n, int window_bits, int checked, int device, zk_msm** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return msm_create(group, bases, n, window_bits, checked, device, out, true);
} ZK_ABI_CATCH
zk_status zk_msm_run(zk_msm* m, const uint8_t* scalars, uint32_t flags, uint8_t* out) try { return msm_run(m, scalars, flags, out); } ZK_ABI_CATCH
zk_status zk_msm_run_dev(zk_msm* m, const void* d_scalars, uint32_t flags, uint8_t* out) try { return msm_run_dev(m, d_scalars, flags, out); } ZK_ABI_CATCH
void zk_msm_free(zk_msm* m) { delete m; }

// (the device this host thread selected last through any other entry, else device 0)
zk_status zk_msm_g1(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    return msm_oneshot(1, bases, scalars, n, out);
} ZK_ABI_CATCH
zk_status zk_msm_g2(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[192]) try {
    return msm_oneshot(2, bases, scalars, n, out);
} ZK_ABI_CATCH

void zk_msm_cache_release(void) {
    std::lock_guard<std::mutex> lock(g_oneshot.mu);
    std::vector<int> keys;
    for (auto& kv : g_oneshot.handles) keys.push_back(kv.first);
    for (int k : keys) {
        if (g_oneshot.handles[k]) (void)use_device(g_oneshot.handles[k]->device);
        oneshot_drop(k);
    }
}
void zk_memory_stats(uint64_t out[6]) {
    if (!out) return;
    out[0] = g_mem.dev_live.load();
    out[1] = g_mem.dev_freed_secret.load();
    out[2] = g_mem.dev_wiped.load();
    out[3] = g_mem.pin_live.load();
    out[4] = g_mem.pin_freed.load();
    out[5] = g_mem.pin_wiped.load();
}

zk_status zk_ntt_create(uint32_t log_n, int device, zk_ntt** out) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    zk_status st = use_device(device);
    if (st != ZK_OK) return st;
    zk_ntt* t = new (std::nothrow) zk_ntt();
    if (!t) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->device = device;
    st = t->plan.init(log_n);
    if (st != ZK_OK) {
        delete t;
        return st;
    }
    *out = t;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_ntt_run_dev(zk_ntt* t, void* d_data, uint32_t batch, uint32_t flags) try { return ntt_run_dev(t, d_data, batch, flags); } ZK_ABI_CATCH
void zk_ntt_free(zk_ntt* t) { delete t; }
#ifdef ZK_TEST_HOOKS
// Test hook, no GPU involved: the launches of one chain of 2^log_n-point transforms (ntt_plan.h).  form = an NttForm, or
// -1: the form the product takes for `batch` transforms under the tile choice of this process, or 0x10 | tiles: the same under
// the tile choice given.  words = [form | per pass: t0, g, log_cw, dif, threads, grid_x, lds_bytes], *n_words of them.
zk_status zk_hook_ntt_plan(uint32_t log_n, uint32_t batch, int dif, int form, uint32_t* words, size_t cap, size_t* n_words) try {
    if (!words || !n_words) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (form == -1) form = ntt_form(NttPlan::tiles(), log_n, batch);
    else if (form >= 0x11 && form <= 0x13) form = ntt_form((NttForm)(form & 3), log_n, batch);
    std::vector<NttLaunch> ps;
    if (!ntt_passes(log_n, dif != 0, 1u << (log_n <= NTT_MAX_LOG ? log_n : 0), form, &ps))
        return fail(ZK_ERR_INVALID_ARGUMENT, "no such tile form for this size");
    *n_words = 1 + 7 * ps.size();
    if (cap < *n_words) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    words[0] = (uint32_t)form;
    for (size_t i = 0; i < ps.size(); i++) {
        const NttLaunch& l = ps[i];
        const uint32_t f[7] = {l.pass.t0, l.pass.g, l.pass.log_cw, l.pass.dif, l.threads, l.grid_x, l.lds_bytes};
        std::copy(f, f + 7, words + 1 + 7 * i);
    }
    return ZK_OK;
} ZK_ABI_CATCH
// (the plan of the size the two hooks below were asked for last: its ten tables are built once for a run of calls)
static zk_status hook_ntt_plan_of(uint32_t log_n, NttPlan** out) {
    static std::unique_ptr<NttPlan> plan;
    ZK_TRY(use_device(0));
    if (!plan || plan->log_n != log_n) {
        plan.reset(new NttPlan());
        const zk_status st = plan->init(log_n);
        if (st != ZK_OK) {
            plan.reset();
            return st;
        }
    }
    *out = plan.get();
    return ZK_OK;
}
// Test hook: NttPlan::chain - the product's, not a copy - on host arrays that the hook uploads and downloads.  data = batch *
// stride elements (stride >= n; back in place), pre / post = n elements, src = batch * src_stride (src_stride >= src_valid),
// minus = batch * minus_stride (minus_stride >= n), each optional; *bad = the flag word after the chain (0 going in).  Only the
// passes [first, first + count) of the chain's list are launched, on whatever state `data` holds.
zk_status zk_hook_ntt_chain(uint32_t log_n, int form, int dif, int inverse, uint32_t batch, uint32_t stride, uint32_t* data,
                            const uint32_t* pre, const uint32_t* post, const uint32_t* src, uint32_t src_stride, uint32_t src_valid,
                            const uint32_t* minus, uint32_t minus_stride, uint32_t first, uint32_t count, uint32_t* bad) try {
    if (!data || !bad) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (log_n > 21 || !batch || batch > 64) return fail(ZK_ERR_INVALID_ARGUMENT, "hook sizes: log_n <= 21, 1 <= batch <= 64");
    const size_t n = (size_t)1 << log_n;
    if (stride < n || ((uint64_t)batch * stride >> 24) || (src && src_stride < src_valid) || (minus && minus_stride < n))
        return fail(ZK_ERR_INVALID_ARGUMENT, "stride shorter than what it holds");
    if (!ntt_form_allowed(form, log_n)) return fail(ZK_ERR_INVALID_ARGUMENT, "no such tile form for this size");
    NttPlan* pl = nullptr;
    ZK_TRY(hook_ntt_plan_of(log_n, &pl));
    DevBuf d_data, d_pre, d_post, d_src, d_minus, d_bad;
    const auto up = [](DevBuf& b, const uint32_t* host, size_t elems) -> zk_status {
        b.is_public = true;
        ZK_TRY(b.ensure(elems * 32 + 32));
        if (host && elems) HIP_TRY(hipMemcpy(b.p, host, elems * 32, hipMemcpyHostToDevice));
        return ZK_OK;
    };
    ZK_TRY(up(d_data, data, (size_t)batch * stride));
    if (pre) ZK_TRY(up(d_pre, pre, n));
    if (post) ZK_TRY(up(d_post, post, n));
    if (src) ZK_TRY(up(d_src, src, (size_t)batch * src_stride));
    if (minus) ZK_TRY(up(d_minus, minus, (size_t)batch * minus_stride));
    ZK_TRY(up(d_bad, nullptr, 0));
    HIP_TRY(hipMemset(d_bad.p, 0, 32));
    const zk_status st = pl->chain((NttForm)form, d_data.as<uint32_t>(), batch, stride, dif != 0, inverse != 0,
                                   pre ? d_pre.as<uint32_t>() : nullptr, post ? d_post.as<uint32_t>() : nullptr,
                                   src ? d_src.as<uint32_t>() : nullptr, src_stride, src_valid, d_bad.as<uint32_t>(),
                                   minus ? d_minus.as<uint32_t>() : nullptr, minus_stride, first, count);
    HIP_TRY(hipStreamSynchronize(g_stream));
    ZK_TRY(st);
    HIP_TRY(hipMemcpy(data, d_data.p, (size_t)batch * stride * 32, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bad, d_bad.p, 4, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: the bytes of one table of NttPlan::init for the domain 2^log_n, which = 0 .. 10: tw_fwd, tw_inv, s1_plain, s1_mont,
// s2, dt, sc_plain, sc_mont, coset_fwd, coset_inv, consts.  *bytes = its length; out == nullptr asks for the length alone.
zk_status zk_hook_ntt_table(uint32_t log_n, uint32_t which, uint8_t* out, size_t cap, size_t* bytes) try {
    if (!bytes || which > 10) return fail(ZK_ERR_INVALID_ARGUMENT, "no such table");
    if (log_n > 21) return fail(ZK_ERR_INVALID_ARGUMENT, "hook sizes: log_n <= 21");
    NttPlan* pl = nullptr;
    ZK_TRY(hook_ntt_plan_of(log_n, &pl));
    const DevBuf* tabs[11] = {&pl->tw_fwd, &pl->tw_inv, &pl->s1_plain, &pl->s1_mont, &pl->s2, &pl->dt,
                              &pl->sc_plain, &pl->sc_mont, &pl->coset_fwd, &pl->coset_inv, &pl->consts};
    *bytes = tabs[which]->cap;   // (what init asked for: a DevBuf holds exactly that)
    if (!out) return ZK_OK;
    if (cap < *bytes) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (*bytes) HIP_TRY(hipMemcpy(out, tabs[which]->p, *bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH
#endif

zk_status zk_ntt_fr(uint8_t* data, uint32_t log_n, int inverse, int coset) try {
    if (!data) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    size_t n = (size_t)1 << log_n;
    zk_status st = check_scalars(data, n, 0);
    if (st != ZK_OK) return st;
    zk_ntt* t = nullptr;
    st = zk_ntt_create(log_n, g_device >= 0 ? g_device : 0, &t);
    if (st != ZK_OK) return st;
    DevBuf buf;
    st = buf.ensure(n * 32);
    if (st == ZK_OK) {
        const unsigned eb = (unsigned)((n + 255) / 256);
        if (hipMemcpy(buf.p, data, n * 32, hipMemcpyHostToDevice) != hipSuccess) st = fail(ZK_ERR_DEVICE, "upload failed");
        if (st == ZK_OK) {
            ZK_LAUNCH(zkdev::k_fr_convert, dim3(eb), dim3(256), 0, g_stream, buf.as<uint32_t>(), buf.as<uint32_t>(), 0u, n);
            st = ntt_run_dev(t, buf.p, 1, (inverse ? ZK_NTT_INVERSE : 0u) | (coset ? ZK_NTT_COSET : 0u));
        }
        if (st == ZK_OK) {
            ZK_LAUNCH(zkdev::k_fr_convert, dim3(eb), dim3(256), 0, g_stream, buf.as<uint32_t>(), buf.as<uint32_t>(), 1u, n);
            if (hipStreamSynchronize(g_stream) != hipSuccess || hipMemcpy(data, buf.p, n * 32, hipMemcpyDeviceToHost) != hipSuccess)
                st = fail(ZK_ERR_DEVICE, "download failed");
        }
    }
    zk_ntt_free(t);
    return st;
} ZK_ABI_CATCH

zk_status zk_debug_field_mul(int field, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) try {
    if (!a || !b || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (field != 0 && field != 1) return fail(ZK_ERR_INVALID_ARGUMENT, "field must be 0 (Fr) or 1 (Fq)");
    zk_status st = use_device(g_device >= 0 ? g_device : 0);
    if (st != ZK_OK || n == 0) return st;
    const size_t sz = field ? 48 : 32;
    DevBuf da, db, dc;
    ZK_TRY(da.ensure(n * sz));
    ZK_TRY(db.ensure(n * sz));
    ZK_TRY(dc.ensure(n * sz));
    HIP_TRY(hipMemcpy(da.p, a, n * sz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db.p, b, n * sz, hipMemcpyHostToDevice));
    dim3 grid((unsigned)((n + 63) / 64));
    if (field)
        ZK_LAUNCH(zkdev::k_field_mul_raw<zkdev::FqCfg>, grid, dim3(64), 0, g_stream, dc.as<uint32_t>(), da.as<uint32_t>(),
                  db.as<uint32_t>(), (uint32_t)n);
    else
        ZK_LAUNCH(zkdev::k_field_mul_raw<zkdev::FrCfg>, grid, dim3(64), 0, g_stream, dc.as<uint32_t>(), da.as<uint32_t>(),
                  db.as<uint32_t>(), (uint32_t)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(out, dc.p, n * sz, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH

void zk_profile_begin(void) {
    zk_profile_end();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof = true;
}
int zk_profile_get(const char* kernel, double* total_ms) {
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int count = 0;
    double tot = 0;
    for (auto& r : g_recs)
        if (!kernel || r.name == kernel) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                tot += ms;
                count++;
            }
        }
    if (total_ms) *total_ms = tot;
    return count;
}
void zk_profile_end(void) {
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_recs.clear();
    g_prof = false;
}
zk_status zk_kernel_forms(int device, uint32_t forms_out[2], float ms_out[4]) try {
    if (device < 0 || device >= 64) return fail(ZK_ERR_INVALID_ARGUMENT, "device index out of range");
    std::lock_guard<std::mutex> lock(g_forms_mu);
    const KernelForms& F = g_forms[device];
    const char* e = getenv("ZKAMD_KERNEL_FORM");
    const int forced = !e ? -1 : !strcmp(e, "free") ? 1 : !strcmp(e, "scratch") ? 0 : -1;
    for (int i = 0; i < 2; i++)
        if (forms_out) forms_out[i] = forced >= 0 ? (uint32_t)forced : F.form[i];
    for (int i = 0; i < 4; i++)
        if (ms_out) ms_out[i] = F.ms[i];
    return ZK_OK;
} ZK_ABI_CATCH
void* zk_stream(void) { return (void*)g_stream; }
zk_status zk_synchronize(void) try {
    if (g_stream) HIP_TRY(hipStreamSynchronize(g_stream));
    if (g_stream2) HIP_TRY(hipStreamSynchronize(g_stream2));
    return ZK_OK;
} ZK_ABI_CATCH

}  // extern "C"
