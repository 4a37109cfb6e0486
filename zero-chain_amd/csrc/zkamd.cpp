// libzkamd: host orchestration + C ABI (include/zkamd.h) of the MI355X Groth16 prover hot path.
//
// What it replaces in the reference (all behind core/proofs/src/confidential.rs:149, in the
// un-vendored bellman 0.1.0 crate; restated in SURVEY.md Appendix A):
//   create_proof step 3  (EvaluationDomain H pipeline)   -> ntt.h kernels, NttPlan below
//   create_proof step 4  (8 x multiexp)                  -> the msm_*.h kernels (overview: msm.h), MsmGroup below
//   create_proof step 6  (final fold, into_affine)       -> k_ct_scale_add (coop_tail.cpp) / k_xyzz_normalize_export (msm_point_kernels.h)
//   Parameters::read                                     -> prover_key.h params_load
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
#if defined(__linux__)
#include <sched.h>
#endif

#include "../../include/zkamd.h"
#include "gpu_rt.h"
#include "host_common.h"
#include "host_math.h"
#include "ntt.h"
#include "r1cs_check.h"
#include "ntt_plan.h"
#include "msm_group.h"
#include "prove_plan.h"
#include "transfer_witness.h"
#include "value_pairs.h"
#include "handles.h"
#include "transfer_r1cs.h"
#include "prover_key.h"
#include "prover_binding.h"

namespace {

// create_proof step 6, rearranged:  with A = alpha + sum_A + r*delta (already
// complete, the alpha and r*delta terms rode along in the A multiexp) and
// C' = h + l + r*(beta_1 + sum_B1) from the merged multiexp,
//   C = s*A + C'   ==  rs*delta + s*alpha + r*beta_1 + s*sum_A + r*sum_B1 + h + l.
// (prove_chunk: the fold and the three into_affine run on the GPU, k_ct_scale_add /
// k_xyzz_normalize_export; the host encodes the 192 bytes.)

// One chunk of proofs: the plan (prove_plan.h), what its stages hand to each other, and the stages in the order they run.
// derived: a, b, c are the library's own row evaluations of the circuit P->bind.drv was built for - the four-transform form over
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
        ZK_TRY(P->work.wit.ensure(np * (size_t)L.wstride * 32));
        wit = P->work.wit.as<uint32_t>();
        ZK_TRY(P->work.pin_tail.ensure(np * 96));
        uint8_t* tail = P->work.pin_tail.as<uint8_t>();
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
        ZK_TRY(P->work.tail.ensure(np * 96));
        HIP_TRY(hipMemcpyAsync(P->work.tail.p, tail, np * 96, hipMemcpyHostToDevice, g_stream));
        ZK_TRY(P->work.bad.ensure(8));
        ZK_TRY(P->work.pin_bad.ensure(8));
        bad = P->work.bad.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(bad, 0, 4, g_stream));
        ZK_TRY(P->work.cvec.ensure(np * (size_t)L.cstride * 32));
        cvec = P->work.cvec.as<uint32_t>();
        const bool bytes = pairs && RUN_W;   // (at RUN_MAX = 2 a pair slot is its pair: nothing to name)
        if (bytes) {   // (every byte is written: by the thread that writes its pair slot)
            ZK_TRY(P->work.sel_w.ensure(np * (size_t)L.sel_w + 1));
            ZK_TRY(P->work.sel_c.ensure(np * (size_t)L.sel_c + 1));
        }
        // (the same launch: a thread per variable, three for the tail, one per group)
        ZK_LAUNCH(zkdev::k_build_scalars, dim3((L.w_end + L.gb1 + 255) / 256, (unsigned)np), dim3(256), 0, g_stream, wit, cvec,
                  (const uint32_t*)bt->d_wit + first * (size_t)nv * 8, P->work.tail.as<uint32_t>(), L, mont ? 1u : 0u, bad,
                  P->maps.grp_dev.as<uint32_t>(), pairs ? (const int32_t*)P->maps.pairs_dev.as<int32_t>() : (const int32_t*)nullptr,
                  bytes ? P->work.sel_w.as<uint8_t>() : (uint8_t*)nullptr, bytes ? P->work.sel_c.as<uint8_t>() : (uint8_t*)nullptr, zkpairs::RUN_MAX);
        return ZK_OK;
    }

    // ---- multiexps (create_proof step 4).  The G2 job only needs the witness scalars: it is
    // enqueued first, on the side stream, and runs beside the H pipeline and the G1 multiexps (its
    // reduction tree is latency-bound with one job per proof; the G1 work fills the machine).
    zk_status g2_set() {
        const uint32_t wstride = plan.layout.wstride;
        P->work.jobs2.clear();
        for (size_t p = 0; p < np; p++) {
            MsmJob j2 = {wit + p * (size_t)wstride * 8, (pairs ? P->maps.map_b2d : P->maps.map_b2).as<int32_t>(), wstride, 0, (uint32_t)G2->n_points, 0, 0, 0};
            P->work.jobs2.push_back(j2);
        }
        HIP_TRY(hipEventRecord(g_ev_fork, g_stream));
        HIP_TRY(hipStreamWaitEvent(side, g_ev_fork, 0));
        // the bytes of the jobs' pair slots: the lengths of their terms pick the bases (msm_types.h MsmSelSet)
        const CJobLayout& L = plan.layout;
        zkdev::MsmSelSet sels = {};
        if (pairs && RUN_W) sels.r[0] = {P->work.sel_w.as<uint8_t>() + L.pa, P->maps.alt_b2.as<int32_t>(), 0u, (uint32_t)np, L.sel_w, L.w_pair_b2, L.pb2, RUN_W};
        ZK_TRY(G2->enqueue(P->work.jobs2, P->work.res2, side, false, &sels));
        ZK_TRY(P->work.pin_g2.ensure(np * sizeof(HG2)));
        if (plan.host_norm) ZK_TRY(G2->export_to_host(G2->res_dev, np, P->work.pin_g2.as<HG2>(), P->work.fold_b2, side));
        else ZK_TRY(G2->normalize_to_host(G2->res_dev, np, P->work.pin_g2.as<HG2>(), P->work.fold_b2, side));   // B in affine form
        return ZK_OK;
    }

    // ---- H pipeline (create_proof step 3): the H block of every C job
    zk_status h_pipeline() {
        const size_t m = P->key.m;
        const uint32_t n_rows = bt->n_rows, cstride = plan.layout.cstride;
        ZK_TRY(P->work.abc.ensure((derived ? 2 : 3) * np * m * 32));
        uint32_t* A = P->work.abc.as<uint32_t>();
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
        const uint32_t* s1 = derived ? P->tab.ntt.dt.as<uint32_t>() : mont ? P->tab.ntt.s1_mont.as<uint32_t>() : P->tab.ntt.s1_plain.as<uint32_t>();
        const uint32_t* sc = mont ? P->tab.ntt.sc_mont.as<uint32_t>() : P->tab.ntt.sc_plain.as<uint32_t>();
        for (int k = 0; k < (derived ? 2 : 3); k++)
            ZK_TRY(P->tab.ntt.chain(P->tab.ntt.form((uint32_t)np), dsts[k], (uint32_t)np, (uint32_t)m, true, true, nullptr, k < 2 ? s1 : sc, srcs[k], n_rows, n_rows, bad));
        // (coset) fft (bit-reversed -> natural) of a and b at once
        ZK_TRY(P->tab.ntt.chain(P->tab.ntt.form((uint32_t)(2 * np)), A, (uint32_t)(2 * np), (uint32_t)m, false, false, nullptr, nullptr));
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
                          (const uint32_t*)B, (const uint32_t*)nullptr, P->tab.ntt.consts.as<uint32_t>() + 8, cvec, (uint32_t)m, cstride, count);
            }
        }
        // icoset fft of a b / (g^m - 1): ifft (natural -> bit-reversed), * g^-i / m, Montgomery factor dropped, minus the
        // scaled coefficients of c (same bit-reversed order); in place inside the merged scalar vectors
        if (!derived)
            ZK_TRY(P->tab.ntt.chain(P->tab.ntt.form((uint32_t)np), cvec, (uint32_t)np, cstride, true, true, nullptr, P->tab.ntt.s2.as<uint32_t>(), nullptr, 0, 0, nullptr,
                                (const uint32_t*)C, (uint32_t)m));
        return ZK_OK;
    }

    // ---- the G1 launch sets (prove_plan.h, split): the C' jobs on the main stream behind the H pipeline and the A jobs on the
    // side stream behind the G2 set, or one set on the main stream - all C' jobs, then all A jobs
    zk_status g1_sets() {
        const bool split = plan.split;
        const uint32_t wstride = plan.layout.wstride, cstride = plan.layout.cstride;
        const uint32_t npts1 = (uint32_t)P->tab.g1.n_points, npts1c = (uint32_t)G1C->n_points;
        P->work.jobs1.clear();
        P->work.jobs1a.clear();
        for (size_t p = 0; p < np; p++) {
            MsmJob jc = {cvec + p * (size_t)cstride * 8, map_c, cstride, 0, npts1c, 0, 0, 0};
            P->work.jobs1.push_back(jc);
        }
        for (size_t p = 0; p < np; p++) {
            MsmJob ja = {wit + p * (size_t)wstride * 8, P->maps.map_a.as<int32_t>(), wstride, P->key.off_a, npts1, 0, 0, 0};
            if (pairs) {   // (absolute positions in the derived table: the pair bases lie in front of its copy of the A query)
                ja.map = P->maps.map_ad.as<int32_t>();
                ja.table_base = 0;
                ja.n_table = (uint32_t)P->bind.g1d.n_points;
            } else if (!split && derived) {   // (one set with the C' jobs: the A query's copy behind the derived bases)
                ja.table_base = P->bind.drv.off_a;
                ja.n_table = npts1c;
            }
            (split ? P->work.jobs1a : P->work.jobs1).push_back(ja);
        }
        // the ranges of jobs whose pair slots follow the bytes (msm_types.h MsmSelSet): the C' jobs, the A jobs
        const CJobLayout& L = plan.layout;
        zkdev::MsmSelSet sc = {}, sa = {};
        if (pairs && RUN_W) {
            sc.r[0] = {P->work.sel_c.as<uint8_t>(), P->maps.alt_c.as<int32_t>(), 0u, (uint32_t)np, L.sel_c, L.pair_l, L.sel_c, RUN_W};
            sa.r[0] = {P->work.sel_w.as<uint8_t>(), P->maps.alt_a.as<int32_t>(), 0u, (uint32_t)np, L.sel_w, L.w_pair_a, L.pa, RUN_W};
            if (!split) {   // (one set: the A jobs behind the C' jobs)
                sc.r[1] = sa.r[0];
                sc.r[1].job0 = (uint32_t)np;
            }
        }
        if (split) {
            MsmG1& G1A = pairs ? P->bind.g1da : P->tab.g1a;
            ZK_TRY(G1A.enqueue(P->work.jobs1a, P->work.res1a, side, false, &sa));
            a_dev = G1A.res_dev;
            HIP_TRY(hipEventRecord(g_ev_join, side));
            ZK_TRY(G1C->enqueue(P->work.jobs1, P->work.res1, g_stream, false, &sc));
            HIP_TRY(hipStreamWaitEvent(g_stream, g_ev_join, 0));   // (a no-op when the side stream is the main one)
        } else {
            ZK_TRY(G1C->enqueue(P->work.jobs1, P->work.res1, g_stream, false, &sc));
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
            ZK_TRY(P->work.fold_tbl.ensure(np * 15 * sizeof(DP1)));
            ZK_TRY(P->work.fold_c.ensure(np * sizeof(DP1)));
            // one row of 16 lanes per proof (coop_tail.cpp): 256 waves, each chain 4 - 5 x shorter than a lane's
            zkcoop::scale_add(a_dev, cprime, (const uint32_t*)P->work.tail.as<uint32_t>() + 16, 24u, P->work.fold_tbl.as<DP1>(),
                              P->work.fold_c.as<DP1>(), (uint32_t)np, g_stream);
            cfin = P->work.fold_c.as<DP1>();
        }
        ZK_TRY(P->work.pin_g1.ensure(2 * np * sizeof(HG1)));
        if (plan.host_norm) {
            ZK_TRY(G1C->export_to_host(a_dev, np, P->work.pin_g1.as<HG1>() + np, P->work.fold_a1, g_stream));
            ZK_TRY(G1C->export_to_host(cfin, np, P->work.pin_g1.as<HG1>(), P->work.fold_c1, g_stream));
        } else {
            ZK_TRY(G1C->normalize2_to_host(a_dev, cfin, np, P->work.pin_g1.as<HG1>() + np, P->work.pin_g1.as<HG1>(), P->work.fold_a1, P->work.fold_c1, g_stream));
        }
        return ZK_OK;
    }

    // ---- wait for the GPU; the flags the kernels raised over the caller's scalars
    zk_status collect(std::chrono::steady_clock::time_point& t_wait) {
        HIP_TRY(hipMemcpyAsync(P->work.pin_bad.p, bad, 8, hipMemcpyDeviceToHost, g_stream));
        t_wait = std::chrono::steady_clock::now();
        ZK_TRY(G1C->collect(g_stream));
        ZK_TRY(G2->collect(side));
        // the reference cannot even represent these assignments (FrRepr -> Fr fails for values >= r,
        // fr.rs:276-289; ProvingAssignment starts with alloc_input(ONE = 1))
        const uint32_t flags = P->work.pin_bad.as<uint32_t>()[0];
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
                const HG1A pa = zkhost::to_affine(P->work.pin_g1.as<HG1>()[np + p]), pc = zkhost::to_affine(P->work.pin_g1.as<HG1>()[p]);
                const HG2A pb = zkhost::to_affine(P->work.pin_g2.as<HG2>()[p]);
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
    if (derived && (!mont || P->bind.drv.n_rows != bt->n_rows)) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: the batch is not the derived set's");
    ChunkRun c = {P, np, bt, first, derived, mont,
                  prove_plan(np, bt->n_inputs, bt->n_aux, bt->n_rows, P->key.m, P->maps.mg_a, P->maps.mg_b2, P->maps.mg_b1, derived, tun, P->maps.mpairs)};
    c.pairs = c.plan.layout.w_b2v != 0;
    c.side = c.plan.one_stream ? g_stream : g_stream2;
    c.G2 = c.pairs ? (c.plan.g2_lone ? &P->bind.g2p_lone : &P->bind.g2p) : (c.plan.g2_lone ? &P->tab.g2_lone : &P->tab.g2);
    MsmG1* const g1s[] = {&P->tab.g1, &P->tab.g1_lone, &P->bind.g1d, &P->bind.g1d_lone};   // in the order of PG1 and PMap
    DevBuf* const maps[] = {&P->maps.map_c, &P->maps.map_cf, &P->maps.map_cd, &P->maps.map_cfd};
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
        if (c.plan.split) ZK_TRY((c.pairs ? P->bind.g1da : P->tab.g1a).count_pairs(np, &pa1));
        ZK_TRY(c.G2->count_pairs(np, &p2));
        fprintf(stderr, "[zkamd] chunk of %zu: pairs per proof: %s %.0f, A set %.0f, G2 set %.0f\n", np, c.plan.split ? "C' set" : "C' and A set",
                (double)pc1 / (double)np, (double)pa1 / (double)np, (double)p2 / (double)np);
    }
    return ZK_OK;
}

zk_status prove_batch_dev(zk_params* P, size_t n, const zk_batch_dev* bt, const uint8_t* rs, uint8_t* proofs_out, bool derived = false) {
    if (!P || !bt || !rs || !proofs_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(P->key.device));
    // bellman create_proof: `if vk.delta_g1.is_zero() || vk.delta_g2.is_zero() { return Err(UnexpectedIdentity) }`
    if (P->key.delta_g1_inf || P->key.delta_g2_inf) return fail(ZK_ERR_UNEXPECTED_IDENTITY, "vk.delta is the point at infinity");
    if (bt->n_inputs == 0) return fail(ZK_ERR_INVALID_ARGUMENT, "n_inputs must include ONE");
    if (bt->n_rows > P->key.m) return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    if (bt->n_inputs != P->key.n_ic) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "number of inputs differs from vk.ic");
    if (bt->n_aux != P->key.n_l) return fail(ZK_ERR_IO, "number of aux variables differs from the l query");
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
    ZK_TRY(use_device(P->key.device));
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
    ZK_TRY(P->work.stage_a.ensure(slots * hc * rb));
    ZK_TRY(P->work.stage_b.ensure(slots * hc * rb));
    ZK_TRY(P->work.stage_c.ensure(slots * hc * rb));
    ZK_TRY(P->work.stage_w.ensure(slots * hc * nvb));
    const hipStream_t copy_stream = g_copy_stream;   // thread-local view: the helper thread gets it by value
    auto stage = [&, copy_stream](size_t slot, size_t first, size_t np) -> zk_status {
        HIP_TRY(hipSetDevice(P->key.device));   // the current device is per host thread
        uint8_t* da = (uint8_t*)P->work.stage_a.p + slot * hc * rb;
        uint8_t* db = (uint8_t*)P->work.stage_b.p + slot * hc * rb;
        uint8_t* dc = (uint8_t*)P->work.stage_c.p + slot * hc * rb;
        uint8_t* dw = (uint8_t*)P->work.stage_w.p + slot * hc * nvb;
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
        bt.d_a = (uint8_t*)P->work.stage_a.p + cur * hc * rb;
        bt.d_b = (uint8_t*)P->work.stage_b.p + cur * hc * rb;
        bt.d_c = (uint8_t*)P->work.stage_c.p + cur * hc * rb;
        bt.d_wit = (uint8_t*)P->work.stage_w.p + cur * hc * nvb;
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
    R->sys.device = device;
    static std::atomic<uint64_t> next_id{1};
    R->sys.id = next_id++;
    R->sys.n_in = n_in;
    R->sys.n_aux = n_aux;
    R->sys.n_con = n_con;
    const uint32_t nv = n_in + n_aux;
    R->sys.a_aux_density.assign(n_aux, 0);
    R->sys.b_input_density.assign(n_in, 0);
    R->sys.b_aux_density.assign(n_aux, 0);
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
            if (m == 0 && v >= n_in) R->sys.a_aux_density[v - n_in] = 1;
            if (m == 1) {
                if (v >= n_in)
                    R->sys.b_aux_density[v - n_in] = 1;
                else
                    R->sys.b_input_density[v] = 1;
            }
        }
        R->sys.h_row_ptr[m].assign(M->row_ptr, M->row_ptr + n_con + 1);
        R->sys.h_col[m].assign(M->col, M->col + nnz);
        R->sys.h_coeff[m].resize(nnz);
        for (uint32_t k = 0; k < nnz; k++) {
            zkhost::Fr c;
            load_scalar_le(M->coeff + (size_t)k * 32, c.l);
            R->sys.h_coeff[m][k] = c.to_mont();
        }
        ZK_TRY(R->sys.row_ptr[m].ensure(((size_t)n_con + 1) * 4));
        ZK_TRY(R->sys.col[m].ensure((size_t)(nnz ? nnz : 1) * 4));
        ZK_TRY(R->sys.coeff[m].ensure((size_t)(nnz ? nnz : 1) * 32));
        HIP_TRY(hipMemcpy(R->sys.row_ptr[m].p, M->row_ptr, ((size_t)n_con + 1) * 4, hipMemcpyHostToDevice));
        if (nnz) {
            HIP_TRY(hipMemcpy(R->sys.col[m].p, M->col, (size_t)nnz * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(R->sys.coeff[m].p, M->coeff, (size_t)nnz * 32, hipMemcpyHostToDevice));
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((nnz + 255) / 256), dim3(256), 0, g_stream, R->sys.coeff[m].as<uint32_t>(),
                      (const uint32_t*)R->sys.coeff[m].as<uint32_t>(), 0u, (size_t)nnz);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    guard.p = nullptr;
    *out = R;
    return ZK_OK;
}

// row evaluations + create_proof of the np assignments in R->work.z[slot] (Montgomery form)
// derived: the caller is one of the statement-to-proof entries, which take the four-transform form over the derived bases
// of the pair (built here the first time); zk_prove_batch_witness keeps the key's own bases
zk_status prove_from_z(zk_params* P, zk_r1cs* R, size_t np, int slot, const uint8_t* rs, uint8_t* proofs_out, bool derived) {
    const uint32_t nv = R->sys.n_in + R->sys.n_aux, n_rows = R->sys.n_con + R->sys.n_in;
    if (derived) {
        ZK_TRY(ensure_derived(P, R, np >= table_multiples_min()));
        derived = P->bind.drv.ready && P->bind.drv.circuit == R->sys.id;
    }
    ZK_TRY(R->work.abc.ensure(3 * np * (size_t)n_rows * 32));
    zkdev::R1csMat mm[3];
    for (int m = 0; m < 3; m++)
        mm[m] = zkdev::R1csMat{R->sys.row_ptr[m].as<uint32_t>(), R->sys.col[m].as<uint32_t>(), R->sys.coeff[m].as<uint32_t>()};
    {
        ProfScope ps("r1cs_eval");
        ZK_LAUNCH(zkdev::k_r1cs_eval, dim3((n_rows + 255) / 256, 3, (unsigned)np), dim3(256), 0, g_stream, mm[0], mm[1], mm[2],
                  (const uint32_t*)R->work.z[slot].as<uint32_t>(), R->work.abc.as<uint32_t>(), R->sys.n_con, R->sys.n_in, nv, n_rows,
                  np * (size_t)n_rows);
    }
    HIP_TRY(hipGetLastError());
    zk_batch_dev bt;
    bt.n_rows = n_rows;
    bt.n_inputs = R->sys.n_in;
    bt.n_aux = R->sys.n_aux;
    bt.flags = ZK_FR_MONTGOMERY;
    bt.d_a = R->work.abc.as<uint32_t>();
    bt.d_b = R->work.abc.as<uint32_t>() + np * (size_t)n_rows * 8;
    bt.d_c = R->work.abc.as<uint32_t>() + 2 * np * (size_t)n_rows * 8;
    bt.d_wit = R->work.z[slot].p;
    bt.a_aux_density = R->sys.a_aux_density.data();
    bt.b_input_density = R->sys.b_input_density.data();
    bt.b_aux_density = R->sys.b_aux_density.data();
    return prove_batch_dev(P, np, &bt, rs, proofs_out, derived);
}

zk_status prove_batch_witness(zk_params* P, zk_r1cs* R, size_t n, const uint8_t* witness, uint32_t flags, const uint8_t* rs,
                              uint8_t* proofs_out, bool derived) {
    if (!P || !R || !witness || !rs || !proofs_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    if (R->sys.device != P->key.device) return fail(ZK_ERR_INVALID_ARGUMENT, "parameters and circuit live on different devices");
    ZK_TRY(use_device(P->key.device));
    const uint32_t nv = R->sys.n_in + R->sys.n_aux, n_rows = R->sys.n_con + R->sys.n_in;
    if (n_rows > P->key.m) return fail(ZK_ERR_POLYNOMIAL_DEGREE_TOO_LARGE, "more rows than the key's evaluation domain");
    const size_t chunk = ProveTunables::read().batch_chunk;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first);
        ZK_TRY(R->work.z[0].ensure(np * (size_t)nv * 32));
        HIP_TRY(hipMemcpyAsync(R->work.z[0].p, witness + first * (size_t)nv * 32, np * (size_t)nv * 32, hipMemcpyHostToDevice, g_stream));
        ZK_TRY(P->work.bad.ensure(8));
        HIP_TRY(hipMemsetAsync(P->work.bad.as<uint32_t>() + 1, 0, 4, g_stream));
        if (!(flags & ZK_FR_MONTGOMERY)) {
            const size_t cnt = np * (size_t)nv;
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, R->work.z[0].as<uint32_t>(),
                      (const uint32_t*)R->work.z[0].as<uint32_t>(), 0u, cnt, P->work.bad.as<uint32_t>() + 1);
        }
        ZK_TRY(prove_from_z(P, R, np, 0, rs + first * 64, proofs_out + first * 192, derived));
        if (P->work.pin_bad.as<uint32_t>()[1] & zkdev::ZK_BAD_SCALAR)
            return fail(ZK_ERR_INVALID_ARGUMENT, "a witness scalar is not a canonical field element (>= r)");
    }
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------
// the constraint check (r1cs_check.h): which row an assignment breaks, with no key and no proof
// ------------------------------------------------------------------------------------------
static_assert(sizeof(zk_r1cs_verdict) == zkdev::R1CS_V_WORDS * 4 && ZK_R1CS_SATISFIED == zkdev::R1CS_SATISFIED &&
                  ZK_R1CS_ONE_IS_NOT_ONE == zkdev::R1CS_ONE_IS_NOT_ONE, "zk_r1cs_verdict as the kernel writes it");
// From this many assignments on the lanes of a wave run across proofs.  Transfer assignments, k_r1cs_check by rows / by proofs
// (profiles/r26_r1cs_check.json): 64: 0.146 / 0.205 ms, 128: 0.243 / 0.272, 256: 0.429 / 0.376, 512: 0.796 / 0.653, 1024:
// 1.643 / 1.402 - a wave per 32 rows of 64 proofs is too few waves for the device below four such groups.
constexpr size_t R1CS_CHECK_LANE_MIN = 256;
#ifdef ZK_TEST_HOOKS
int g_r1cs_check_mapping = -1;   // tools/r1cs_check_probe.py: 0 / 1 force a mapping, -1 the rule above
#endif

// R->work.verdict = [16 bytes: the flags k_fr_convert raises over a caller's scalars | one verdict per assignment]
zk_status verdict_ensure(zk_r1cs* R, size_t np) { return R->work.verdict.ensure((np + 1) * sizeof(zk_r1cs_verdict)); }

// the verdicts of the np assignments in R->work.z[slot] (Montgomery form), on the host when this returns
zk_status check_from_z(zk_r1cs* R, size_t np, int slot, zk_r1cs_verdict* out) {
    const uint32_t nv = R->sys.n_in + R->sys.n_aux, n_con = R->sys.n_con;
    ZK_TRY(verdict_ensure(R, np));
    uint32_t* const verdict = R->work.verdict.as<uint32_t>() + zkdev::R1CS_V_WORDS;
    const uint32_t* z = R->work.z[slot].as<uint32_t>();
    zkdev::R1csMat mm[3];
    for (int m = 0; m < 3; m++)
        mm[m] = zkdev::R1csMat{R->sys.row_ptr[m].as<uint32_t>(), R->sys.col[m].as<uint32_t>(), R->sys.coeff[m].as<uint32_t>()};
    ZK_LAUNCH(zkdev::k_r1cs_check_begin, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, g_stream, z, nv, (uint32_t)np, verdict);
    bool lanes = np >= R1CS_CHECK_LANE_MIN;
#ifdef ZK_TEST_HOOKS
    if (g_r1cs_check_mapping >= 0) lanes = g_r1cs_check_mapping != 0;
#endif
    if (n_con) {
        ProfScope ps("r1cs_check");
        if (lanes)
            ZK_LAUNCH(zkdev::k_r1cs_check<true>, dim3((n_con + zkdev::R1CS_CHECK_ROWS - 1) / zkdev::R1CS_CHECK_ROWS,
                                                      (unsigned)((np + zkdev::R1CS_CHECK_WAVE - 1) / zkdev::R1CS_CHECK_WAVE)),
                      dim3(zkdev::R1CS_CHECK_WAVE), 0, g_stream, mm[0], mm[1], mm[2], z, verdict, n_con, nv, (uint32_t)np);
        else
            ZK_LAUNCH(zkdev::k_r1cs_check<false>, dim3((n_con + 255) / 256, (unsigned)np), dim3(256), 0, g_stream, mm[0], mm[1], mm[2], z,
                      verdict, n_con, nv, (uint32_t)np);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(out, verdict, np * sizeof(zk_r1cs_verdict), hipMemcpyDeviceToHost));
    return ZK_OK;
}

// zk_r1cs_check_batch: prove_batch_witness with check_from_z in the place of prove_from_z - the same chunks, R->work.z[0], the
// same refusal of a scalar >= r (own: the host calculator's vectors, canonical by construction, as prove_statements hands them on)
zk_status check_batch_witness(zk_r1cs* R, size_t n, const uint8_t* witness, uint32_t flags, zk_r1cs_verdict* out, bool own) {
    if (!R || (n && (!witness || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return ZK_OK;
    ZK_TRY(use_device(R->sys.device));
    const uint32_t nv = R->sys.n_in + R->sys.n_aux;
    const size_t chunk = ProveTunables::read().batch_chunk;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t np = std::min(chunk, n - first), cnt = np * (size_t)nv;
        ZK_TRY(R->work.z[0].ensure(cnt * 32));
        ZK_TRY(verdict_ensure(R, np));
        uint32_t* const bad = R->work.verdict.as<uint32_t>();
        HIP_TRY(hipMemcpyAsync(R->work.z[0].p, witness + first * (size_t)nv * 32, cnt * 32, hipMemcpyHostToDevice, g_stream));
        HIP_TRY(hipMemsetAsync(bad, 0, 4, g_stream));
        if (!(flags & ZK_FR_MONTGOMERY))
            ZK_LAUNCH(zkdev::k_fr_convert, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream, R->work.z[0].as<uint32_t>(),
                      (const uint32_t*)R->work.z[0].as<uint32_t>(), 0u, cnt, bad);
        else if (!own)
            ZK_LAUNCH(zkdev::k_fr_flag_noncanonical, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, g_stream,
                      (const uint32_t*)R->work.z[0].as<uint32_t>(), cnt, bad);
        ZK_TRY(check_from_z(R, np, 0, out + first));
        uint32_t raised = 0;
        HIP_TRY(hipMemcpy(&raised, bad, 4, hipMemcpyDeviceToHost));
        if (raised & zkdev::ZK_BAD_SCALAR)
            return fail(ZK_ERR_INVALID_ARGUMENT, "a witness scalar is not a canonical field element (>= r)");
    }
    return ZK_OK;
}

}  // namespace

#include "statement_route.h"   // (the statement route: host witness calculators, route_check, prove_statements, ...)
#include "pipeline.h"          // (zk_pipeline: its lanes over the route's witness engines)

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
    // the encodings are decoded on the device (msm_point_kernels.h k_decode_uncompressed: 0.1 ms for 2^20 points, the host loop it
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
// gen_proof's chunks: statement_chunks over the transfer circuit with the typed inputs tested by the witness kernels; after each
// chunk is proved, packed(first, np, heads, head_stride) gets the 23 public inputs of every statement of it (the head of its
// assignment, Montgomery form), for check_proof and the packing.  since: where ZKAMD_DEBUG_TIMING counts from (null: no prints).
zk_status lib_transfer_chunks(zk_params* P, zk_r1cs* R, size_t n, const zk_transfer_statement* st, const uint8_t* rs, uint8_t* proofs_out,
                              const TransferChunkPacked& packed, const std::chrono::steady_clock::time_point* since) {
    const size_t chunk = ProveTunables::read().batch_chunk, nv = ZK_TRANSFER_N_INPUTS + ZK_TRANSFER_N_AUX, head = ZK_TRANSFER_N_INPUTS * 32;
    PinBuf pin_in;
    struct WipeHalves {   // (the assignments hold the bits of the keys: both halves of the host engine, on every way out)
        zk_r1cs* R;
        size_t bytes;
        ~WipeHalves() {
            if (R->work.host_z) explicit_bzero(R->work.host_z, std::min(bytes, R->work.host_z_cap));
        }
    } wipe{R, witness_on_host(n) ? 2 * std::min(chunk, n) * nv * 32 : 0};
    return statement_chunks(R, zkpairs::TRANSFER, st, n, [&](size_t first, size_t np, int slot, const uint8_t* host_z) -> zk_status {
        if (host_z) {
            // derived = false, the key's own bases: a lone transaction must not pay the binding of the derived bases
            // (ensure_derived) on its first call
            ZK_TRY(prove_batch_witness(P, R, np, host_z, ZK_FR_MONTGOMERY, rs + first * 64, proofs_out + first * 192, false));
            return packed(first, np, host_z, nv * 32);
        }
        ZK_TRY(pin_in.ensure(std::min(chunk, n) * head));
        HIP_TRY(hipMemcpy2DAsync(pin_in.p, head, R->work.z[slot].p, nv * 32, head, np, hipMemcpyDeviceToHost, g_stream));
        if (since)
            fprintf(stderr, "[gen_proof] chunk %zu witness ready %.1f ms\n", first / chunk,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - *since).count());
        ZK_TRY(prove_from_z(P, R, np, slot, rs + first * 64, proofs_out + first * 192, true));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return packed(first, np, pin_in.as<uint8_t>(), head);
    }, true);
}
bool lib_witness_on_host(size_t n) { return witness_on_host(n); }
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
    info->n_ic = p->key.n_ic;
    info->n_h = p->key.n_h;
    info->n_l = p->key.n_l;
    info->n_a = p->key.n_a;
    info->n_b_g1 = p->key.n_b1;
    info->n_b_g2 = p->key.n_b2;
    info->log_domain = p->key.log_m;
    info->window_bits = p->tab.g1.c;
    info->n_windows = zkdev::MSM_NPOS;
    info->device = (uint32_t)p->key.device;
    info->device_bytes = p->tab.g1.bytes + p->tab.g2.bytes + p->tab.ntt.bytes;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_windows(const zk_params* p, uint32_t out[4]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = p->tab.g1.c;
    out[1] = p->tab.g1a.c;
    out[2] = p->tab.g1_lone.c;
    out[3] = p->tab.g2.c;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_merged(const zk_params* p, uint32_t out[3]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = p->key.grp_a.merged();
    out[1] = p->key.grp_b1.merged();
    out[2] = p->key.grp_b2.merged();
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_params_get_pairs(const zk_params* p, uint32_t out[8]) try {
    if (!p || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    const zk_params::Binding::Pairs& X = p->bind.prs;
    const uint32_t v[8] = {X.q[QA].n, X.q[QB1].n, X.q[QB2].n, X.q[QL].n, X.q[QA].expect, X.q[QB1].expect, X.q[QB2].expect, X.q[QL].expect};
    for (int i = 0; i < 8; i++) out[i] = p->bind.drv.ready && X.ready ? v[i] : 0u;
    return ZK_OK;
} ZK_ABI_CATCH
void zk_params_free(zk_params* p) { delete p; }
zk_status zk_params_write_vk(const zk_params* p, uint8_t* out, size_t cap, size_t* len) try {
    if (!p || !len) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *len = p->key.vk_bytes.size();
    if (out) {
        if (cap < p->key.vk_bytes.size()) return fail(ZK_ERR_INVALID_ARGUMENT, "output buffer too small");
        memcpy(out, p->key.vk_bytes.data(), p->key.vk_bytes.size());
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

// the natively emitted constraint systems of the two circuits (statement_route.h)
zk_status zk_transfer_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints) try {
    return system_fingerprint(zkpairs::TRANSFER, hash_out, n_inputs, n_aux, n_constraints);
} ZK_ABI_CATCH
zk_status zk_transfer_r1cs_load(int device, zk_r1cs** out) try {
    return system_load(zkpairs::TRANSFER, device, out);
} ZK_ABI_CATCH
zk_status zk_anonymous_r1cs_fingerprint(uint8_t hash_out[32], uint32_t* n_inputs, uint32_t* n_aux, uint32_t* n_constraints) try {
    return system_fingerprint(zkpairs::ANONYMOUS, hash_out, n_inputs, n_aux, n_constraints);
} ZK_ABI_CATCH
zk_status zk_anonymous_r1cs_load(int device, zk_r1cs** out) try {
    return system_load(zkpairs::ANONYMOUS, device, out);
} ZK_ABI_CATCH
zk_status zk_prove_batch_witness(zk_params* p, zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags,
                                 const uint8_t* rs, uint8_t* proofs_out) try {
    return prove_batch_witness(p, circuit, n, witness, flags, rs, proofs_out, false);   // (a caller's witness: the key's own bases)
} ZK_ABI_CATCH
// Which constraint an assignment breaks (r1cs_check.h; statement_route.h check_statements).  A verdict is not an error.
zk_status zk_r1cs_check_batch(zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags, zk_r1cs_verdict* out) try {
    return check_batch_witness(circuit, n, witness, flags, out, false);
} ZK_ABI_CATCH
zk_status zk_transfer_check_batch(zk_r1cs* circuit, size_t n, const zk_transfer_statement* st, zk_r1cs_verdict* out) try {
    if (!circuit || (n && (!st || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(nullptr, circuit, zkpairs::TRANSFER, n));
    return n ? check_statements(circuit, zkpairs::TRANSFER, st, n, out) : ZK_OK;
} ZK_ABI_CATCH
zk_status zk_anonymous_check_batch(zk_r1cs* circuit, size_t n, const zk_anonymous_statement* st, zk_r1cs_verdict* out) try {
    if (!circuit || (n && (!st || !out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(nullptr, circuit, zkpairs::ANONYMOUS, n));
    return n ? check_statements(circuit, zkpairs::ANONYMOUS, st, n, out) : ZK_OK;
} ZK_ABI_CATCH
// the part of a built-in circuit a constraint belongs to (transfer_r1cs.h System::mark; system_load hands the table on)
zk_status zk_r1cs_stage(const zk_r1cs* circuit, uint32_t constraint, uint32_t* stage_out, uint32_t* first_out, uint32_t* count_out,
                        char* name_out, size_t name_cap) try {
    if (!circuit) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    const zk_r1cs::System& S = circuit->sys;
    if (constraint >= S.n_con)
        return fail(ZK_ERR_INVALID_ARGUMENT, "constraint " + std::to_string(constraint) + " of " + std::to_string(S.n_con));
    uint32_t stage = 0xFFFFFFFFu, first = 0, count = S.n_con;
    const char* name = "";
    if (!S.stage_first.empty()) {
        stage = (uint32_t)(std::upper_bound(S.stage_first.begin(), S.stage_first.end(), constraint) - S.stage_first.begin()) - 1;
        first = S.stage_first[stage];
        count = (stage + 1 < S.stage_first.size() ? S.stage_first[stage + 1] : S.n_con) - first;
        name = S.stage_name[stage].c_str();
    }
    if (stage_out) *stage_out = stage;
    if (first_out) *first_out = first;
    if (count_out) *count_out = count;
    if (name_out && name_cap) {
        strncpy(name_out, name, name_cap - 1);
        name_out[name_cap - 1] = 0;
    }
    return ZK_OK;
} ZK_ABI_CATCH
#ifdef ZK_TEST_HOOKS
// Test hooks of tools/r1cs_check_probe.py, NOT part of the ABI: the lane mapping of the check forced (0 rows, 1 proofs, -1 the
// library's rule); the check, and the row evaluations of the prover, on the np assignments a call left in R->work.z[0] -
// each under its zk_profile name ("r1cs_check", "r1cs_eval").
zk_status zk_hook_r1cs_check_mapping(int mapping) try {
    g_r1cs_check_mapping = mapping;
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_hook_r1cs_check_resident(zk_r1cs* circuit, size_t np, zk_r1cs_verdict* out) try {
    if (!circuit || !out || !np) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(circuit->sys.device));
    if (circuit->work.z[0].cap < np * (size_t)(circuit->sys.n_in + circuit->sys.n_aux) * 32)
        return fail(ZK_ERR_INVALID_ARGUMENT, "fewer assignments are resident");
    return check_from_z(circuit, np, 0, out);
} ZK_ABI_CATCH
zk_status zk_hook_r1cs_eval_resident(zk_r1cs* circuit, size_t np) try {
    if (!circuit || !np) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    zk_r1cs* R = circuit;
    ZK_TRY(use_device(R->sys.device));
    const uint32_t nv = R->sys.n_in + R->sys.n_aux, n_rows = R->sys.n_con + R->sys.n_in;
    if (R->work.z[0].cap < np * (size_t)nv * 32) return fail(ZK_ERR_INVALID_ARGUMENT, "fewer assignments are resident");
    ZK_TRY(R->work.abc.ensure(3 * np * (size_t)n_rows * 32));
    zkdev::R1csMat mm[3];
    for (int m = 0; m < 3; m++)
        mm[m] = zkdev::R1csMat{R->sys.row_ptr[m].as<uint32_t>(), R->sys.col[m].as<uint32_t>(), R->sys.coeff[m].as<uint32_t>()};
    {
        ProfScope ps("r1cs_eval");
        ZK_LAUNCH(zkdev::k_r1cs_eval, dim3((n_rows + 255) / 256, 3, (unsigned)np), dim3(256), 0, g_stream, mm[0], mm[1], mm[2],
                  (const uint32_t*)R->work.z[0].as<uint32_t>(), R->work.abc.as<uint32_t>(), R->sys.n_con, R->sys.n_in, nv, n_rows,
                  np * (size_t)n_rows);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook, NOT part of the ABI (absent from libzkamd.so): zk_prove_batch_witness on the route of the statement-to-proof
// entries - the four-transform form over the derived bases of (p, circuit) - for circuits that have no statement form.
// info[0] = whether the pair has a derived set after the call, info[1] = how many of its bases are the identity (mapped out).
zk_status zk_hook_prove_batch_witness_derived(zk_params* p, zk_r1cs* circuit, size_t n, const uint8_t* witness, uint32_t flags,
                                              const uint8_t* rs, uint8_t* proofs_out, uint32_t info[2]) try {
    const zk_status rc = prove_batch_witness(p, circuit, n, witness, flags, rs, proofs_out, true);
    if (info && p && circuit) {
        info[0] = p->bind.drv.ready && p->bind.drv.circuit == circuit->sys.id ? 1u : 0u;
        info[1] = (uint32_t)std::count(p->bind.drv.pos.begin(), p->bind.drv.pos.end(), -1);
    }
    return rc;
} ZK_ABI_CATCH
// Test hook: the layout of the derived set (p, circuit) carries, [Lambda | E | D | a | alpha_1 | delta_1 | b_g1 | beta_1].
// info = [has a set, terms of the H block, of the residual block, of the variables, offset of the A query's copy, of the
// b_g1 query's, recoding width of the set], zeros behind info[0] without one.
zk_status zk_hook_derived_layout(zk_params* p, zk_r1cs* circuit, uint32_t info[7]) try {
    if (!p || !circuit || !info) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::fill(info, info + 7, 0u);
    const zk_params::Binding::Derived& D = p->bind.drv;
    if (!D.ready || D.circuit != circuit->sys.id) return ZK_OK;
    info[0] = 1;
    info[1] = info[2] = D.n_rows;
    info[3] = (uint32_t)D.pos.size() - 2 * D.n_rows;
    info[4] = D.off_a;
    info[5] = D.off_b1;
    info[6] = p->bind.g1d.c;
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
    const PairCounts pc = PairCounts::of(counts);
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
    const zkr1cs::System& sys = builtin_system((zkpairs::Circuit)circuit);
    const uint32_t nv = sys.n_inputs + sys.n_aux;
    if (nv_out) *nv_out = nv;
    if (!out) return ZK_OK;
    if (cap < 8 * (size_t)nv) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    std::vector<uint8_t> a_dense, b_dense;
    system_densities(sys, a_dense, b_dense);
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
    const PairCounts pc = PairCounts::of(counts);
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
            const int32_t* pred = links + 2 * (size_t)nv * zkpairs::chain_of((Query)k);
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
    const zk_params::Binding::Pairs& X = p->bind.prs;
    if (!p->bind.drv.ready || !X.ready) return fail(ZK_ERR_INVALID_ARGUMENT, "the key has no value pairs");
    const uint32_t nv = (uint32_t)(X.links.size() / 11);
    const uint32_t f[12] = {zkpairs::RUN_MAX, nv, X.q[QA].n, X.q[QB2].n, X.q[QL].n, X.q[QB1].n, X.q[QA].xbase, X.q[QB2].xbase, X.q[QL].xbase, X.q[QB1].xbase,
                            (uint32_t)X.hook_g1.size(), (uint32_t)X.hook_g2.size()};
    std::copy(f, f + 12, info);
    if (!links) return ZK_OK;
    if (!alt || !g1 || !g2 || !d) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::copy(X.links.begin(), X.links.end(), links);
    for (const auto& Q : X.q) alt = std::copy(Q.alt.begin(), Q.alt.end(), alt);
    for (size_t i = 0; i < X.hook_g1.size(); i++) zkhost::g1_to_uncompressed(X.hook_g1[i], g1 + i * 96);
    for (size_t i = 0; i < X.hook_g2.size(); i++) zkhost::g2_to_uncompressed(X.hook_g2[i], g2 + i * 192);
    for (size_t i = 0; i < X.hook_d.size(); i++) zkhost::g1_to_uncompressed(X.hook_d[i], d + i * 96);
    return ZK_OK;
} ZK_ABI_CATCH
// Test hook: n_jobs multiexp jobs over the bases of a G1 handle, each of n scalars (plain words) through one map, with the
// bytes and alternates of msm_types.h MsmSelRange over the slots [sel_first, sel_first + sel_n) (sel: sel_n bytes per job, or
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
// Statement -> proof (statement_route.h prove_statements): the witnesses of chunk k + 1 - the witness kernels on the side
// stream, or the native host calculator on the host cores (witness_on_host) - beside the proving of chunk k.  Both engines
// prove every chunk before the first malformed statement's and report that statement in the same words.
zk_status zk_transfer_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_transfer_statement* st,
                                  const uint8_t* rs, uint8_t* proofs_out) try {
    if (!p || !circuit || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(p, circuit, zkpairs::TRANSFER, n));
    return n ? prove_statements(p, circuit, zkpairs::TRANSFER, st, n, rs, proofs_out) : ZK_OK;
} ZK_ABI_CATCH
// ... for the anonymous-transfer circuit (core/proofs/src/anonymous.rs:165: create_random_proof of AnonymousTransfer)
zk_status zk_anonymous_prove_batch(zk_params* p, zk_r1cs* circuit, size_t n, const zk_anonymous_statement* st, const uint8_t* rs,
                                   uint8_t* proofs_out) try {
    if (!p || !circuit || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(route_check(p, circuit, zkpairs::ANONYMOUS, n));
    return n ? prove_statements(p, circuit, zkpairs::ANONYMOUS, st, n, rs, proofs_out) : ZK_OK;
} ZK_ABI_CATCH

// The witness vectors the GPU generators produce, copied back to the host (tests: element by element against zk_transfer_witness
// / zk_anonymous_witness).  witness_out: n x (23 + 19955) x 32 bytes / n x (105 + 50429) x 32 bytes.
zk_status zk_transfer_witness_gpu(zk_r1cs* circuit, const zk_transfer_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    return witness_readback(circuit, zkpairs::TRANSFER, st, n, flags, witness_out);
} ZK_ABI_CATCH
zk_status zk_anonymous_witness_gpu(zk_r1cs* circuit, const zk_anonymous_statement* st, size_t n, uint32_t flags, uint8_t* witness_out) try {
    return witness_readback(circuit, zkpairs::ANONYMOUS, st, n, flags, witness_out);
} ZK_ABI_CATCH

// ------------------------------------------------------------------------------------------
// zk_pipeline: a stream of statement batches (pipeline.h)
// ------------------------------------------------------------------------------------------
zk_status zk_pipeline_create(zk_params* p, zk_r1cs* circuit, zk_pipeline** out) try {
    if (!p || !circuit || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    ZK_TRY(route_check(p, circuit, zkpairs::TRANSFER));
    (void)zkwit::tables();
    // the derived bases of the pair before the lanes borrow the key's tables: every lane binds to the same set
    ZK_TRY(ensure_derived(p, circuit, true));
    zk_pipeline* L = new (std::nothrow) zk_pipeline();
    if (!L) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    L->Pl[0] = p;
    L->Rl[0] = circuit;
    L->chunk = ProveTunables::read().batch_chunk;
    L->host = witness_on_host();
    int lanes = 1;   // (the host calculator: lane 0 alone)
    if (!L->host) {
        lanes = 2;
        if (const char* env = getenv("ZKAMD_PIPELINE_LANES")) lanes = atoi(env);
#ifdef ZK_EMU
        lanes = 1;   // the test-only emulation runs one launch at a time
#endif
        if (lanes > zk_pipeline::MAX_LANES) lanes = zk_pipeline::MAX_LANES;
        // Every lane allocates its chunk workspaces the first time it proves (~36 MB per proof of a transfer-circuit chunk:
        // 35 GB at 1024).  The free memory seen here only caps the number of lanes STARTED (a hint: it is check-then-
        // allocate, and another process may take the memory in between); it never refuses the pipeline - lane 0 lets the
        // real allocation report OutOfMemory, and a further lane whose allocation fails later hands its jobs back and
        // retires (pipeline_lanes.h lane_run).  A zk_params that has proved before already holds lane 0's workspaces.
#ifndef ZK_EMU
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            size_t per_lane = L->chunk * ((size_t)36 << 20);
            if (const char* env = getenv("ZKAMD_LANE_BYTES"))
                if (atoll(env) > 0) per_lane = (size_t)atoll(env);
            const size_t reserve = (size_t)2 << 30;
            const size_t avail = free_b > reserve ? free_b - reserve : 0;
            const size_t lane0 = p->work.abc.p ? 0 : per_lane;       // nothing more to allocate once it has proved a chunk
            const size_t fit = 1 + (avail > lane0 ? (avail - lane0) / per_lane : 0);
            if ((size_t)lanes > fit) lanes = (int)fit;
        }
#endif
    }
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
    L->Q.open(L->n_lanes);
    try {
        for (int l = 0; l < L->n_lanes; l++)
            L->t_lane[l] = std::thread([L, l] {
                PipelineLane lane{L, l};
                zkpipe::lane_run(L->Q, l, lane);
            });
    } catch (const std::system_error& e) {
        zk_pipeline_free(L);
        return fail(ZK_ERR_OUT_OF_MEMORY, std::string("cannot start a pipeline worker: ") + e.what());
    }
    *out = L;
    return ZK_OK;
} ZK_ABI_CATCH

int zk_pipeline_lanes(const zk_pipeline* L) { return L ? L->Q.lanes() : 0; }

zk_status zk_pipeline_submit(zk_pipeline* L, size_t n, const zk_transfer_statement* st, const uint8_t* rs, uint8_t* proofs_out) try {
    if (!L || !rs || !proofs_out || (!st && n)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<zkpipe::Job> jobs;
    for (size_t first = 0; first < n; first += L->chunk)
        jobs.push_back(zkpipe::Job{st + first, rs + first * 64, proofs_out + first * 192, std::min(L->chunk, n - first), first});
    L->Q.submit(jobs.data(), jobs.size());
    return ZK_OK;
} ZK_ABI_CATCH

zk_status zk_pipeline_wait(zk_pipeline* L) try {
    if (!L) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return L->Q.wait(&g_err);
} ZK_ABI_CATCH

void zk_pipeline_free(zk_pipeline* L) {
    if (!L) return;
    L->Q.close();
    for (int l = 0; l < zk_pipeline::MAX_LANES; l++) {
        if (L->t_lane[l].joinable()) L->t_lane[l].join();
        if (l) delete L->Pl[l];   // (lane 0 works on the caller's handles)
        if (l) delete L->Rl[l];
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

#include "msm_hooks.h"   // (test hooks of the table multiples: -DZK_TEST_HOOKS only)
