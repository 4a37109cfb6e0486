// The G1 instantiation of the MSM group (msm_group.h): its kernels - the generated assembly loops of the accumulation and of
// level 1 of the bucket reduction among them - are compiled here and nowhere else.  So are the kernels of the sort and of the
// task order, which both groups run through msm_sort_pairs / msm_order_tasks below.
#define ZK_MSM_GROUP_INSTANTIATE 1
#include "msm_group_impl.h"
#include "msm_sort.h"
#include "msm_asm_g1.h"

namespace zkrt {

zk_status msm_sort_pairs(const MsmPlan& p, hipStream_t st, const MsmSortBufs& w, uint32_t nb, uint32_t c, const zkdev::MsmRecode& rc,
                         const zkdev::MsmSelSet& sel_set) {
    const size_t nj = p.nj;
    const MsmJob* dj = w.jobs;
    if (p.lds_sort) {
        // histogram + scan + scatter of a job inside one workgroup's LDS
        ProfScope ps("msm_sort_lds", st);
        ZK_LAUNCH_SYNC(zkdev::k_msm_sort_lds, dim3((unsigned)nj), dim3(zkdev::MSM_SORT_THREADS), (size_t)nb * 4, st, dj, c, w.cnt, w.off, w.toff,
                       w.ntasks, w.pairs, p.seg, hook_env("ZKAMD_DEBUG_SORT") ? (uint32_t)atoi(hook_env("ZKAMD_DEBUG_SORT")) : 0u, sel_set, rc);
        return ZK_OK;
    }
    // two-level counting sort, every per-digit atomic in LDS (msm_sort.h)
    const uint32_t fine_log = p.fine_log, fine = 1u << fine_log, n_coarse = p.n_coarse, per_wg = zkdev::MSM_COARSE_SCALARS;
    const dim3 gridc(p.coarse_wgs, (unsigned)nj);
    uint32_t* coarse_cnt = w.coarse;
    uint32_t* coarse_off = coarse_cnt + nj * (size_t)n_coarse;
    uint32_t* bin_tasks = coarse_off + nj * (size_t)n_coarse;
    uint32_t* bin_tbase = bin_tasks + nj * (size_t)n_coarse;
    HIP_TRY(hipMemsetAsync(coarse_cnt, 0, nj * (size_t)n_coarse * 4, st));
    {
        ProfScope ps("msm_sort_coarse", st);
        ZK_LAUNCH_SYNC(zkdev::k_msm_coarse_count, gridc, dim3(256), 0, st, dj, c, fine_log, n_coarse, coarse_cnt, w.blockbase, per_wg, sel_set, rc);
        ZK_LAUNCH_SYNC(zkdev::k_msm_coarse_scan, dim3((unsigned)nj), dim3(zkdev::MSM_SORT_THREADS), 0, st,
                       (const uint32_t*)coarse_cnt, coarse_off, (uint32_t*)nullptr, n_coarse);
        ZK_LAUNCH_SYNC(zkdev::k_msm_coarse_scatter, gridc, dim3(256), 0, st, dj, c, fine_log, n_coarse,
                       (const uint32_t*)coarse_off, (const uint32_t*)w.blockbase, w.rank, per_wg, sel_set, rc);
    }
    {
        ProfScope ps("msm_sort_fine", st);
        ZK_LAUNCH_SYNC(zkdev::k_msm_fine_sort, dim3(n_coarse, (unsigned)nj), dim3(zkdev::MSM_SORT_THREADS), 0, st, dj,
                       (const uint2*)w.rank, (const uint32_t*)coarse_cnt, (const uint32_t*)coarse_off, fine, nb, w.cnt, w.off, w.toff,
                       bin_tasks, w.pairs, p.seg);
        ZK_LAUNCH_SYNC(zkdev::k_msm_coarse_scan, dim3((unsigned)nj), dim3(zkdev::MSM_SORT_THREADS), 0, st,
                       (const uint32_t*)bin_tasks, bin_tbase, w.ntasks, n_coarse);
        ZK_LAUNCH(zkdev::k_msm_task_offsets, dim3((nb + 255) / 256, (unsigned)nj), dim3(256), 0, st, w.toff,
                  (const uint32_t*)bin_tbase, nb, fine_log, n_coarse);
    }
    return ZK_OK;
}

zk_status msm_order_tasks(const MsmPlan& p, hipStream_t st, const MsmSortBufs& w, uint32_t nb) {
    const uint32_t nj = (uint32_t)p.nj;
    const dim3 gridb((nb + 255) / 256, nj);
    uint32_t* lenhist = w.hist;
    uint32_t* cursor = lenhist + p.n_class;
    ProfScope ps("msm_task_sort", st);
    ZK_LAUNCH_SYNC(zkdev::k_msm_task_hist, gridb, dim3(256), 0, st, w.cnt, lenhist, nb, p.seg);
    ZK_LAUNCH_SYNC(zkdev::k_msm_task_base, dim3(1), dim3(zkdev::MSM_SORT_THREADS), 0, st, lenhist, w.tclass, w.n_tasks, nj, p.seg);
    ZK_LAUNCH_SYNC(zkdev::k_msm_task_place, gridb, dim3(256), 0, st, w.cnt, w.off, w.toff, w.tbase, w.tclass, cursor, w.sorted, w.n_heavy,
                   w.heavy, nb, nj, p.merge_inline, p.seg, w.n_light, w.light);
    return ZK_OK;
}

#ifdef ZK_HAVE_RED_ASM
template <>
void launch_red_asm<zkdev::Fq28>(const zkdev::XYZZ<zkdev::Fq28>* tsums, const uint32_t* cnt, const uint32_t* toff, const uint32_t* tbase,
                                 zkdev::XYZZ<zkdev::Fq28>* S, zkdev::XYZZ<zkdev::Fq28>* A, uint32_t nb, uint32_t L, dim3 grid,
                                 hipStream_t st, uint32_t* n_fallback, uint32_t* fallback) {
    if (kernel_form(1)) {
        // the scratch-free form lists the nodes with a special case; the compiled addition takes them in a second launch
        ZK_LAUNCH(zkdev::k_msm_reduce1_g1asm_sf, grid, dim3(64), 0, st, tsums, cnt, toff, tbase, S, A, nb, L, n_fallback, fallback);
        ZK_LAUNCH(zkdev::k_msm_reduce1_redo, dim3(256), dim3(64), 0, st, tsums, cnt, toff, tbase, S, A, nb, L, (const uint32_t*)n_fallback,
                  (const uint32_t*)fallback);
    } else {
        ZK_LAUNCH(zkdev::k_msm_reduce1_g1asm, grid, dim3(64), 0, st, tsums, cnt, toff, tbase, S, A, nb, L, n_fallback);
    }
}
#endif
#ifdef ZK_HAVE_MADD_ASM
// workgroups per CU of the persistent form of the G1 loop (0 = one workgroup per 128 tasks, the plain launch)
int persist_wgs(int group) {
    static const int v1 = getenv("ZKAMD_G1_PERSIST") ? atoi(getenv("ZKAMD_G1_PERSIST")) : 6;
    static const int v2 = getenv("ZKAMD_G2_PERSIST") ? atoi(getenv("ZKAMD_G2_PERSIST")) : 4;
    return group == 2 ? v2 : v1;
}
template <>
void launch_asm_loop<zkdev::Fq28>(const zkdev::Affine<zkdev::Fq28>* table, const uint32_t* pairs, const uint4* sorted,
                                  const uint32_t* d_total, zkdev::XYZZ<zkdev::Fq28>* tsums, uint32_t* d_nredo, uint32_t* redo,
                                  unsigned blocks, hipStream_t st) {
    if (persist_wgs() > 0 && blocks > 256u * (unsigned)persist_wgs())
        ZK_LAUNCH(zkdev::k_msm_accumulate_g1asm_persistent, dim3(256u * (unsigned)persist_wgs()), dim3(128), 0, st, table, pairs, sorted,
                  d_total, tsums, d_nredo, redo, d_nredo + 1);
    else
        ZK_LAUNCH(zkdev::k_msm_accumulate_g1asm, dim3(blocks), dim3(128), 0, st, table, pairs, sorted, d_total, tsums, d_nredo, redo);
    ZK_LAUNCH_SYNC(zkdev::k_msm_accumulate_redo<zkdev::Fq28>, dim3(1024), dim3(64), 0, st, table, pairs, sorted,
                   (const uint32_t*)d_nredo, (const uint32_t*)redo, tsums);
}
#endif

zk_status calibrate_g1_reduce(const zkdev::Affine<zkdev::Fq28>* table, uint32_t n1, float ms[2]) {
#ifdef ZK_HAVE_RED_ASM
    // level 1 of the G1 reduction: 256 jobs of 4 096 buckets in nodes of 8 = 131 072 threads, one machine of waves
    typedef zkdev::XYZZ<zkdev::Fq28> P1;
    const uint32_t nj = 256, nb = 4096, L = 8, T = nb / L, n_sums = 1u << 16;
    DevBuf sums, cnt, toff, tbase, S, A, ctr, list;
    ZK_TRY(sums.ensure((size_t)n_sums * sizeof(P1)));
    ZK_TRY(cnt.ensure((size_t)nj * nb * 4));
    ZK_TRY(toff.ensure((size_t)nj * nb * 4));
    ZK_TRY(tbase.ensure(nj * 4));
    ZK_TRY(S.ensure((size_t)nj * T * sizeof(P1)));
    ZK_TRY(A.ensure((size_t)nj * T * sizeof(P1)));
    ZK_TRY(ctr.ensure(4));
    ZK_TRY(list.ensure((size_t)nj * T * 4));
    HIP_TRY(hipMemsetAsync(tbase.p, 0, nj * 4, g_stream));
    ZK_LAUNCH(zkdev::k_calib_buckets<zkdev::Fq28>, dim3(nj * nb / 256), dim3(256), 0, g_stream, table, n1, sums.as<P1>(), n_sums,
              cnt.as<uint32_t>(), toff.as<uint32_t>(), nj * nb);
    const dim3 grid(T / 64, nj);
    ZK_TRY(timed_best([&] {
        (void)hipMemsetAsync(ctr.p, 0, 4, g_stream);
        ZK_LAUNCH(zkdev::k_msm_reduce1_g1asm, grid, dim3(64), 0, g_stream, (const P1*)sums.as<P1>(), (const uint32_t*)cnt.as<uint32_t>(),
                  (const uint32_t*)toff.as<uint32_t>(), (const uint32_t*)tbase.as<uint32_t>(), S.as<P1>(), A.as<P1>(), nb, L, ctr.as<uint32_t>());
    }, &ms[0]));
    ZK_TRY(timed_best([&] {
        (void)hipMemsetAsync(ctr.p, 0, 4, g_stream);
        ZK_LAUNCH(zkdev::k_msm_reduce1_g1asm_sf, grid, dim3(64), 0, g_stream, (const P1*)sums.as<P1>(), (const uint32_t*)cnt.as<uint32_t>(),
                  (const uint32_t*)toff.as<uint32_t>(), (const uint32_t*)tbase.as<uint32_t>(), S.as<P1>(), A.as<P1>(), nb, L, ctr.as<uint32_t>(),
                  list.as<uint32_t>());
        ZK_LAUNCH(zkdev::k_msm_reduce1_redo, dim3(256), dim3(64), 0, g_stream, (const P1*)sums.as<P1>(), (const uint32_t*)cnt.as<uint32_t>(),
                  (const uint32_t*)toff.as<uint32_t>(), (const uint32_t*)tbase.as<uint32_t>(), S.as<P1>(), A.as<P1>(), nb, L,
                  (const uint32_t*)ctr.as<uint32_t>(), (const uint32_t*)list.as<uint32_t>());
    }, &ms[1]));
    HIP_TRY(hipStreamSynchronize(g_stream));
#else
    (void)table; (void)n1;
    ms[0] = ms[1] = 0.f;
#endif
    return ZK_OK;
}

ZK_MSM_GROUP_DEFINE(zkhost::Fq, zkdev::Fq)

}  // namespace zkrt

#ifdef ZK_TEST_HOOKS
// Test hook, NOT part of the ABI (absent from libzkamd.so): the plan of the launch set that n_jobs jobs of n[k] scalars each
// would be in a group of window c (msm_plan.h; vb_digit != 0: the digit positions of a variable-base multiexp), under the
// environment of the call.  has_asm_loop / has_asm_reduce stand for the build (the emulation has neither loop, the product
// both).  out[0 .. 48) = the plan's fields in the order of the list below, then n_jobs x pair_base, n_jobs x tbase; a
// refused set returns the refusal, its wording in zk_last_error().
extern "C" zk_status zk_hook_msm_plan(int is_g2, uint32_t c, const uint32_t* n, size_t n_jobs, uint32_t vb_digit, int has_asm_loop,
                                      int has_asm_reduce, uint64_t* out, size_t out_words) try {
    using namespace zkrt;
    if (!n || !n_jobs || !out || c < 2 || c > 22) return fail(ZK_ERR_INVALID_ARGUMENT, "bad argument");
    std::vector<MsmJob> jobs(n_jobs, MsmJob{});
    for (size_t k = 0; k < n_jobs; k++) {
        jobs[k].n = n[k];
        jobs[k].vb_digit = vb_digit;
    }
    MsmPlan p;
    if (msm_plan(p, is_g2 != 0, c, 1u << (c - 2), vb_digit ? 1u : zkdev::msm_max_digits(c), jobs.data(), n_jobs, has_asm_loop != 0,
                 has_asm_reduce != 0, MsmTunables::read(is_g2 != 0)) != ZK_OK)
        return fail(p.status, p.refusal);
    const MsmPlan::Bytes& b = p.bytes;
    const uint64_t f[] = {p.seg, p.few, p.coop_l1, p.coop_rb, p.merge_inline, p.heavy_cap, p.light_cap, p.use_light, p.big_launch, p.acc_asm,
                          p.red_asm, p.L, p.T, p.nbits, p.log2_2l, p.s_stride, p.nsplit, p.lds_sort, p.fine_log, p.n_coarse, p.coarse_wgs,
                          p.heavy_blocks, p.medium_max, p.max_n, p.total, p.total_tasks, p.n_buckets, p.n_class,
                          b.jobs_d, b.bucket, b.per_job, b.hist, b.heavy, b.light, b.tclass, b.sorted, b.tsums, b.pairs, b.red_r, b.red_w, b.red_t,
                          b.pin_jobs, b.rank, b.blockbase, b.coarse, b.redo, b.result, n_jobs};
    const size_t nf = sizeof(f) / sizeof(f[0]);
    if (out_words < nf + 2 * n_jobs) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    std::copy(f, f + nf, out);
    std::copy(p.pair_base.begin(), p.pair_base.end(), out + nf);
    std::copy(p.tbase.begin(), p.tbase.end(), out + nf + n_jobs);
    return ZK_OK;
} ZK_ABI_CATCH
#endif
