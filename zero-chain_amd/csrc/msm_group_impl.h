// The member functions of MsmGroup (msm_group.h) that launch kernels: included by msm_g1.cpp and msm_g2.cpp only, so that no
// other unit instantiates - and compiles - the ~25 kernels each of them pulls in.  The passes both groups launch are included
// here; the sort (msm_sort.h) and the wrappers of the generated loops (msm_asm_g1.h / msm_asm_g2.h) by the one unit that
// launches them.
#pragma once
#include "msm_group.h"
#include "msm_accumulate.h"
#include "msm_reduce.h"
#include "msm_point_kernels.h"

namespace zkrt {

template <class DF>
zk_status import_affine_dev(const void* d_src, zkdev::Affine<DF>* dst, size_t n, hipStream_t st) {
    if (!n) return ZK_OK;
    ZK_LAUNCH(zkdev::k_import_affine<DF>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, (const uint32_t*)d_src, dst, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class DF>
zk_status build_table_dev(zkdev::Affine<DF>* table, size_t n, uint32_t npos, DevBuf& scratch, uint32_t n_mult, uint32_t j0, hipStream_t st) {
    ZK_TRY(scratch.ensure((size_t)zkdev::MSM_TABLE_CHUNK * 5 * sizeof(DF) * n));   // chunk of un-normalised slices + prefix products
    ZK_LAUNCH(zkdev::k_msm_build_table<DF>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, table, (uint32_t)n, npos, scratch.as<DF>(),
              n_mult, j0);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class HF, class DF>
zk_status check_points_dev(const zkdev::Affine<DF>* d_pts, size_t n, const char* what) {
    if (!n) return ZK_OK;
    DevBuf flags;
    ZK_TRY(flags.ensure(4 * n));
    ZK_LAUNCH(zkdev::k_check_points<DF>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, g_stream, d_pts, (uint32_t)n, 1u,
              flags.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> f(n);
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(f.data(), flags.p, 4 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        if (f[i])
            return fail(ZK_ERR_IO, std::string(what) + ": point " + std::to_string(i) +
                                       (f[i] & 1 ? " is not on the curve" : " is not in the correct subgroup"));
    return ZK_OK;
}
template <class HF, class DF>
zk_status check_points_host(const std::vector<zkhost::Affine<HF>>& pts, const char* what) {
    if (pts.empty()) return ZK_OK;
    DevBuf stage, d;
    ZK_TRY(stage.ensure(pts.size() * sizeof(zkhost::Affine<HF>)));
    ZK_TRY(d.ensure(pts.size() * sizeof(zkdev::Affine<DF>)));
    HIP_TRY(hipMemcpy(stage.p, pts.data(), pts.size() * sizeof(zkhost::Affine<HF>), hipMemcpyHostToDevice));
    ZK_TRY(import_affine_dev<DF>(stage.p, d.as<zkdev::Affine<DF>>(), pts.size(), g_stream));
    zk_status st = check_points_dev<HF, DF>(d.as<zkdev::Affine<DF>>(), pts.size(), what);
    HIP_TRY(hipStreamSynchronize(g_stream));
    return st;
}


// one machine-filling launch, three times, the first not counted: the best of the other two in ms (the load-time
// comparisons of msm_g1.cpp / msm_g2.cpp)
template <class Launch>
zk_status timed_best(Launch&& launch, float* best) {
    hipEvent_t ev[2];
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            (void)hipEventDestroy(e[0]);
            (void)hipEventDestroy(e[1]);
        }
    } evg{ev};
    *best = 1e30f;
    for (int rep = 0; rep < 3; rep++) {   // (the first repetition warms the instruction cache and is not counted)
        HIP_TRY(hipEventRecord(ev[0], g_stream));
        launch();
        HIP_TRY(hipEventRecord(ev[1], g_stream));
        HIP_TRY(hipEventSynchronize(ev[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        if (rep && ms < *best) *best = ms;
    }
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::decode_enqueue(const uint8_t* bases, size_t n, uint32_t c_, bool with_table, DevBuf& raw, DevBuf& map, hipStream_t st) {
    ZK_TRY(set_geometry(c_, n, with_table));
    table.is_public = true;   // bases of a key or of a multiexp: public points, 4.2 GB for the transfer key - freed without the wipe
    ZK_TRY(table.ensure(bytes ? bytes : 1));
    ZK_TRY(dstat.ensure(8));
    HIP_TRY(hipMemsetAsync(dstat.p, 0xff, 4, st));
    HIP_TRY(hipMemsetAsync((uint8_t*)dstat.p + 4, 0, 4, st));
    if (!n) return ZK_OK;
    const size_t enc = sizeof(HAffine);   // 96 / 192: an uncompressed encoding is as long as the host's affine point
    ZK_TRY(raw.ensure(enc * n));
    ZK_TRY(map.ensure(4 * n));
    HIP_TRY(hipMemcpyAsync(raw.p, bases, enc * n, hipMemcpyHostToDevice, st));
    ZK_LAUNCH(zkdev::k_decode_uncompressed<DF>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, (const uint32_t*)raw.as<uint32_t>(),
              table.as<DAffine>(), map.as<int32_t>(), dstat.as<uint32_t>(), (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::launch_table_build(DevBuf& scratch, hipStream_t st) {
    return build_table_dev<DF>(table.as<DAffine>(), n_points, zkdev::MSM_NPOS, scratch, n_mult, 0u, st);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::add_multiples(uint32_t n_mult_) {
    if (n_mult_ <= n_mult || !n_points) return ZK_OK;
    if (n_mult != 1 || !table.owned || n_mult_ > zkdev::MSM_MULT_MAX) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: multiples cannot be added to this table");
    if ((uint64_t)n_points * zkdev::MSM_NPOS * n_mult_ >= (1ull << 31)) return fail(ZK_ERR_INVALID_ARGUMENT, "doubling table too large");
    const size_t one = sizeof(DAffine) * n_points * zkdev::MSM_NPOS;
    DevBuf grown, scratch;
    grown.is_public = true;
    ZK_TRY(grown.ensure(one * n_mult_));
    HIP_TRY(hipMemcpyAsync(grown.p, table.p, one, hipMemcpyDeviceToDevice, g_stream));
    ZK_TRY(build_table_dev<DF>(grown.as<DAffine>(), n_points, zkdev::MSM_NPOS, scratch, n_mult_, 1u, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    std::swap(table.p, grown.p);       // (the table with one multiple goes with `grown`)
    std::swap(table.cap, grown.cap);
    set_multiples(n_mult_);
    bytes = one * n_mult_;
    return ensure_recode();
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::ensure_recode() {
    if (n_mult <= 1 || lut.p) return ZK_OK;
    std::vector<uint8_t> h((size_t)1 << (c + ext - 1));
    for (size_t v = 0; v < h.size(); v++) h[v] = zkdev::msm_mult_choice((uint32_t)(2 * v + 1), c, n_mult, ext);
    lut.is_public = true;   // a function of (c, n_mult, ext) alone
    return lut.upload(h);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::table_enqueue(DevBuf& scratch, hipStream_t st) {
    return n_points ? launch_table_build(scratch, st) : ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::finish_build(bool checked, const char* what, bool with_table) {
    if (!n_points) return ZK_OK;
    if (checked) ZK_TRY((check_points_dev<HF, DF>(table.as<DAffine>(), n_points, what)));
    if (with_table) {
        DevBuf scratch;   // freed after the build
        ZK_TRY(launch_table_build(scratch, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        ZK_TRY(ensure_recode());
    }
    return ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::build(const std::vector<typename MsmGroup<HF, DF>::HAffine>& pts, uint32_t c_, bool checked, const char* what, bool with_table,
                                  uint32_t n_mult_) {
    ZK_TRY(set_geometry(c_, pts.size(), with_table, n_mult_));
    table.is_public = true;   // bases of a key or of a multiexp: public points, 4.2 GB for the transfer key - freed without the wipe
    ZK_TRY(table.ensure(bytes ? bytes : 1));
    if (!n_points) return ZK_OK;
    {
        DevBuf stage;
        ZK_TRY(stage.ensure(sizeof(HAffine) * n_points));
        HIP_TRY(hipMemcpy(stage.p, pts.data(), sizeof(HAffine) * n_points, hipMemcpyHostToDevice));
        ZK_TRY(import_affine_dev<DF>(stage.p, table.as<DAffine>(), n_points, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
    }
    return finish_build(checked, what, with_table);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::build_with_tail(const std::vector<typename MsmGroup<HF, DF>::HAffine>& pts, const MsmGroup& o, size_t from,
                                            size_t count, uint32_t c_, uint32_t n_mult_) {
    if (from + count > o.n_points) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: tail outside the borrowed table");
    ZK_TRY(set_geometry(c_, pts.size() + count, true, n_mult_));
    table.is_public = true;   // images of a key's bases under public maps
    ZK_TRY(table.ensure(bytes ? bytes : 1));
    if (!pts.empty()) {
        DevBuf stage;
        stage.is_public = true;
        ZK_TRY(stage.ensure(sizeof(HAffine) * pts.size()));
        HIP_TRY(hipMemcpy(stage.p, pts.data(), sizeof(HAffine) * pts.size(), hipMemcpyHostToDevice));
        ZK_TRY(import_affine_dev<DF>(stage.p, table.as<DAffine>(), pts.size(), g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
    }
    if (count)
        HIP_TRY(hipMemcpy(table.as<DAffine>() + pts.size(), o.table.template as<DAffine>() + from, sizeof(DAffine) * count, hipMemcpyDeviceToDevice));
    return finish_build(false, "derived bases", true);
}

// One launch set: plan (msm_plan.h: every decision about its shape, nothing enqueued before a refusal), then the stages
// below in this order.
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::enqueue(std::vector<MsmJob>& jobs, std::vector<typename MsmGroup<HF, DF>::HPoint>& out, hipStream_t st, bool to_host,
                                    const zkdev::MsmSelSet* sels) {
    const size_t nj = jobs.size();
    out.resize(nj);
    res_dev = nullptr;
    if (!nj) return ZK_OK;
    MsmPlan p;
    if (msm_plan(p, IS_G2, c, nb, maxd, jobs.data(), nj, asm_loop<DF>(), asm_reduce<DF>(), MsmTunables::read(IS_G2)) != ZK_OK)
        return fail(p.status, p.refusal);
    for (size_t k = 0; k < nj; k++) jobs[k].pair_base = p.pair_base[k];
    ZK_TRY(ensure_recode());
    ZK_TRY(reserve(p, to_host));
    ZK_TRY(upload_jobs(jobs, p, st));
    ZK_TRY(sort_pairs(p, st, sels ? *sels : zkdev::MsmSelSet{}));
    if (hook_env("ZKAMD_DEBUG_PAIRS")) dump_pairs(jobs[0], st, hook_env("ZKAMD_DEBUG_PAIRS"));
    ZK_TRY(order_tasks(p, st));
    ZK_TRY(accumulate(p, st));
    {
        ProfScope ps(IS_G2 ? "msm_reduce_g2" : "msm_reduce_g1", st);
        ZK_TRY(merge_partials(p, st));   // ts[0] of every bucket with several task partials = their sum
        ZK_TRY(level1(p, st));           // S and W of every node of L buckets
        ZK_TRY(tail(p, st));             // sums[j] = sum_t W_t + 2 L sum_t t S_t over the T nodes of job j
    }
    res_dev = job_sums(p);   // one XYZZ per job, valid until the next enqueue on this group
    if (to_host) return export_to_host(res_dev, nj, out.data(), result, st);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::reserve(const MsmPlan& p, bool to_host) {
    const MsmPlan::Bytes& b = p.bytes;
    const std::pair<DevBuf*, size_t> workspaces[] = {
        {&jobs_d, b.jobs_d}, {&cnt, b.bucket}, {&off, b.bucket}, {&toff, b.bucket}, {&ntasks, b.per_job}, {&tbase, b.per_job},
        {&hist, b.hist}, {&heavy, b.heavy}, {&light, b.light}, {&tclass, b.tclass}, {&sorted, b.sorted}, {&tsums, b.tsums},
        {&pairs, b.pairs}, {&red_r, b.red_r}, {&red_w, b.red_w}, {&red_t, b.red_t}, {&rank, b.rank}, {&blockbase, b.blockbase},
        {&coarse, b.coarse}, {&redo, b.redo}};
    for (const auto& w : workspaces) ZK_TRY(w.first->ensure(w.second));
    ZK_TRY(pin_jobs.ensure(b.pin_jobs));
    if (to_host) ZK_TRY(result.ensure(b.result));
    return ZK_OK;
}

// job descriptors through page-locked staging (collect() separates consecutive launch sets); the counters start at zero
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::upload_jobs(const std::vector<MsmJob>& jobs, const MsmPlan& p, hipStream_t st) {
    const size_t nj = p.nj;
    memcpy(pin_jobs.p, jobs.data(), nj * sizeof(MsmJob));
    memcpy((uint8_t*)pin_jobs.p + nj * sizeof(MsmJob), p.tbase.data(), nj * 4);
    HIP_TRY(hipMemcpyAsync(jobs_d.p, pin_jobs.p, nj * sizeof(MsmJob), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tbase.p, (const uint8_t*)pin_jobs.p + nj * sizeof(MsmJob), nj * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(hist.p, 0, p.bytes.hist, st));
    return ZK_OK;
}

// the sort and the task order: the group's workspaces handed to the plain functions of msm_g1.cpp (msm_group.h)
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::sort_pairs(const MsmPlan& p, hipStream_t st, const zkdev::MsmSelSet& sel_set) {
    return msm_sort_pairs(p, st, sort_bufs(p), nb, c, recode(), sel_set);
}
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::order_tasks(const MsmPlan& p, hipStream_t st) {
    return msm_order_tasks(p, st, sort_bufs(p), nb);
}

// tsums[t] = the sum of the points of task t
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::accumulate(const MsmPlan& p, hipStream_t st) {
    ProfScope ps(IS_G2 ? "msm_accumulate_g2" : "msm_accumulate_g1", st);
    const unsigned blocks = (unsigned)((p.total_tasks + 127) / 128);
    if (p.acc_asm) {
        // the generated assembly loop (msm_asm_g1.h / msm_asm_g2.h, madd_asm.h), then the compiled loop over the few tasks it flagged
        launch_asm_loop(table.as<DAffine>(), pairs.as<uint32_t>(), sorted.as<uint4>(), counter(p, N_TASKS), tsums.as<DPoint>(),
                        counter(p, N_REDO), redo.as<uint32_t>(), blocks, st);
        if (hook_env("ZKAMD_DEBUG_REDO")) dump_redo(p, st, false);
    } else if constexpr (IS_G2)   // G2: one wave per SIMD with the whole register file
        ZK_LAUNCH(zkdev::k_msm_accumulate_wide<DF>, dim3(blocks), dim3(128), 0, st, table.as<DAffine>(), pairs.as<uint32_t>(),
                  sorted.as<uint4>(), counter(p, N_TASKS), tsums.as<DPoint>());
    else
        ZK_LAUNCH(zkdev::k_msm_accumulate<DF>, dim3(blocks), dim3(128), 0, st, table.as<DAffine>(), pairs.as<uint32_t>(),
                  sorted.as<uint4>(), counter(p, N_TASKS), tsums.as<DPoint>());
    return ZK_OK;
}

// merge: ts[0] of every bucket with several task partials = their sum
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::merge_partials(const MsmPlan& p, hipStream_t st) {
    const uint32_t seg = p.seg, merge_inline = p.merge_inline, heavy_blocks = p.heavy_blocks;
    const bool few = p.few;
    uint32_t* d_nheavy = counter(p, N_HEAVY);
    if (p.coop_l1) {
        // on rows of 16 lanes (coop_tail.cpp)
        zkcoop::merge<DF>(heavy.as<uint32_t>(), d_nheavy, cnt.as<uint32_t>(), toff.as<uint32_t>(), tbase.as<uint32_t>(),
                          tsums.as<DPoint>(), nb, seg, p.n_buckets, heavy_blocks, merge_inline, p.coop_rb, st);
        return ZK_OK;
    }
    // on lanes.  A few jobs: the buckets with many partials (the top digit position of a variable-base multiexp:
    // 2^(c-6) buckets with dozens of tasks each) take a workgroup of rows each all the same - 64 partials are 8
    // additions of 9 us there, 7 of 43+ us on lanes (the 2^17-point G2 multiexp: profiles/r06z_*) - the listed
    // buckets with up to MEDIUM_MAX partials eight lanes each (k_msm_merge_medium: the list of a variable-base
    // multiexp can hold half of its buckets), and the buckets with 2 .. merge_inline partials one lane each in the
    // trailing workgroups of k_msm_merge_heavy
    // (MEDIUM_MAX: msm_plan.h medium_max)
    const uint32_t MEDIUM_MAX = p.medium_max;
    if (hook_env("ZKAMD_DEBUG_HEAVY")) dump_heavy(p, st);
    const uint32_t min_heavy = few ? MEDIUM_MAX : 0u;
    if (few) {
        ZK_LAUNCH_SYNC(zkdev::k_msm_merge_medium<DF>, dim3((unsigned)std::min<size_t>((p.heavy_cap + 7) / 8, 4096)), dim3(64), 0, st,
                       (const uint32_t*)heavy.as<uint32_t>(), (const uint32_t*)d_nheavy, (const uint32_t*)cnt.as<uint32_t>(),
                       (const uint32_t*)toff.as<uint32_t>(), (const uint32_t*)tbase.as<uint32_t>(), tsums.as<DPoint>(), nb, seg, MEDIUM_MAX);
        zkcoop::merge<DF>(heavy.as<uint32_t>(), d_nheavy, cnt.as<uint32_t>(), toff.as<uint32_t>(), tbase.as<uint32_t>(),
                          tsums.as<DPoint>(), nb, seg, 0, heavy_blocks, merge_inline, 1, st, min_heavy);
    }
    // a chunk of proofs: the heavy list, one workgroup of lanes per bucket ...
    const uint32_t lane_heavy_blocks = few ? 0u : heavy_blocks;
    const uint32_t light_buckets = few ? (uint32_t)p.n_buckets : 0u;
    ZK_LAUNCH_SYNC(zkdev::k_msm_merge_heavy<DF>,
                   dim3(lane_heavy_blocks + (light_buckets + zkdev::MSM_MERGE_THREADS - 1) / zkdev::MSM_MERGE_THREADS),
                   dim3(zkdev::MSM_MERGE_THREADS), 0, st, (const uint32_t*)heavy.as<uint32_t>(), (const uint32_t*)d_nheavy,
                   (const uint32_t*)cnt.as<uint32_t>(), (const uint32_t*)toff.as<uint32_t>(),
                   (const uint32_t*)tbase.as<uint32_t>(), tsums.as<DPoint>(), nb, seg, lane_heavy_blocks, light_buckets,
                   merge_inline, min_heavy);
    // ... and the listed buckets with 2 .. merge_inline partials, one thread each: level 1 then meets ONE partial
    // per bucket
    if (p.use_light)
        ZK_LAUNCH_SYNC(zkdev::k_msm_merge_light<DF>, dim3((unsigned)std::min<size_t>((p.light_cap + 63) / 64, 2048)), dim3(64), 0, st,
                       (const uint32_t*)light.as<uint32_t>(), (const uint32_t*)counter(p, N_LIGHT), (const uint32_t*)cnt.as<uint32_t>(),
                       (const uint32_t*)toff.as<uint32_t>(), (const uint32_t*)tbase.as<uint32_t>(), tsums.as<DPoint>(), nb, seg);
    return ZK_OK;
}

// level 1: S and W of every node of L buckets
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::level1(const MsmPlan& p, hipStream_t st) {
    const uint32_t nj = (uint32_t)p.nj, L = p.L;
    const dim3 grid((p.T + 63) / 64, nj);   // a thread per node
    DPoint *R = node_s(), *W = node_w();
    if (p.coop_l1) {
        zkcoop::level1<DF>(tsums.as<DPoint>(), cnt.as<uint32_t>(), toff.as<uint32_t>(), tbase.as<uint32_t>(), R, W, nb, L, nj, st);
    } else if (p.red_asm) {
        // in assembly: S = R_0 and, in W's place, A = sum_{k>=1} R_k = (W - S) / 2
        launch_red_asm<DF>(tsums.as<DPoint>(), cnt.as<uint32_t>(), toff.as<uint32_t>(), tbase.as<uint32_t>(), R, W, nb, L, grid, st,
                           counter(p, N_FALLBACK), redo.as<uint32_t>());
        if (hook_env("ZKAMD_DEBUG_REDO")) dump_redo(p, st, true);
    } else {
        // on lanes: R = suffix sums over the buckets of a node; S = R_0; W = 2 * sum_{k>=1} R_k + R_0
        ZK_LAUNCH(zkdev::k_msm_suffix_buckets<DF>, grid, dim3(64), 0, st, tsums.as<DPoint>(), cnt.as<uint32_t>(),
                  toff.as<uint32_t>(), tbase.as<uint32_t>(), R, nb, L, p.few ? 0u : 1u /* merged by now */, p.seg);
        ZK_LAUNCH(zkdev::k_msm_segsum<DF>, grid, dim3(64), 0, st, (const DPoint*)R, (const DPoint*)nullptr, W, nb, L,
                  1u, 1u, 1u);
    }
    return ZK_OK;
}

// tail: sums[j] = sum_t W_t + 2 L sum_t t S_t over the T nodes of job j, on rows of 16 lanes (coop_tail.cpp)
template <class HF, class DF>
zk_status MsmGroup<HF, DF>::tail(const MsmPlan& p, hipStream_t st) {
    const uint32_t nj = (uint32_t)p.nj, nbits = p.nbits;
    if (p.few) {
        // folded at once: bit planes, then their weighted sum - chains of ~15 and ~20 dependent additions of 2 - 4 us
        DPoint* parts = red_t.as<DPoint>();    // [nj (nbits + 1) nsplit] when a plane takes several workgroups
        DPoint* Y = p.nsplit > 1 ? parts + p.nj * (size_t)(nbits + 1) * p.nsplit : parts;   // [nj (nbits + 1)]
        zkcoop::planes<DF>(node_s(), p.s_stride, node_w(), Y, parts, p.T, nbits, nj, st);
        zkcoop::combine<DF>(Y, job_sums(p), nbits, p.log2_2l, nj, st);
    } else {
        // a chunk of proofs: one workgroup per job walks its nodes (three additions per node, not (nbits + 1) / 2)
        zkcoop::upper<DF>(node_s(), p.s_stride, node_w(), job_sums(p), p.T, p.log2_2l, p.red_asm, nj, st);
    }
    return ZK_OK;
}

// diagnostics: how many tasks went to the second pass of the accumulation, and what they look like; after level 1 in
// assembly: the nodes it handed to the compiled addition
template <class HF, class DF>
void MsmGroup<HF, DF>::dump_redo(const MsmPlan& p, hipStream_t st, bool after_level1) {
    (void)hipStreamSynchronize(st);
    if (after_level1) {
        uint32_t v[2] = {0, 0};
        (void)hipMemcpy(v, counter(p, N_LIGHT), 8, hipMemcpyDeviceToHost);
        fprintf(stderr, "[redo] reduction G1: %u buckets with 2..%u partials merged, %u of %zu level-1 nodes recomputed\n", v[0],
                p.merge_inline, v[1], p.nj * (size_t)p.T);
        return;
    }
    uint32_t nr = 0, tot = 0;
    (void)hipMemcpy(&nr, counter(p, N_REDO), 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&tot, counter(p, N_TASKS), 4, hipMemcpyDeviceToHost);
    fprintf(stderr, "[redo] group %s: %u of %u tasks flagged\n", IS_G2 ? "G2" : "G1", nr, tot);
    for (uint32_t q = 0; q < nr && q < 6; q++) {
        uint32_t ti = 0;
        uint4 dsc;
        (void)hipMemcpy(&ti, redo.as<uint32_t>() + q, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&dsc, sorted.as<uint4>() + ti, 16, hipMemcpyDeviceToHost);
        std::vector<uint32_t> pw(dsc.z);
        (void)hipMemcpy(pw.data(), pairs.as<uint32_t>() + dsc.x, dsc.z * 4, hipMemcpyDeviceToHost);
        std::sort(pw.begin(), pw.end());
        uint32_t dup = 0, opp = 0;
        for (size_t u = 1; u < pw.size(); u++) {
            dup += pw[u] == pw[u - 1];
            opp += (pw[u] ^ pw[u - 1]) == 1u;
        }
        fprintf(stderr, "[redo]   task %u: n = %u, equal pair words %u, opposite pair words %u, first %u %u %u\n", ti, dsc.z, dup, opp,
                pw.size() > 0 ? pw[0] : 0, pw.size() > 1 ? pw[1] : 0, pw.size() > 2 ? pw[2] : 0);
    }
}

// diagnostics: the first job of the first launch set of every width - its scalars, its map and the pairs the sort counted for
// it - into <dir>/pairs_<g1|g2>_c<width>.bin = [c, n_mult, ext, n, pairs, has map | n x 8 words | n map entries], so that the
// count can be held against a recoding of the same scalars made elsewhere (profiles/r28_table_multiples.txt)
template <class HF, class DF>
void MsmGroup<HF, DF>::dump_pairs(const MsmJob& job0, hipStream_t st, const char* dir) {
    static uint32_t seen = 0;
    if (job0.vb_digit || c >= 32 || (seen >> c & 1u)) return;
    seen |= 1u << c;
    (void)hipStreamSynchronize(st);
    std::vector<uint32_t> h(nb), sc((size_t)job0.n * 8);
    std::vector<int32_t> mp(job0.map ? job0.n : 0);
    (void)hipMemcpy(h.data(), cnt.p, (size_t)nb * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(sc.data(), job0.scalars, sc.size() * 4, hipMemcpyDeviceToHost);
    if (job0.map) (void)hipMemcpy(mp.data(), job0.map, mp.size() * 4, hipMemcpyDeviceToHost);
    uint32_t pairs_job0 = 0;
    for (uint32_t x : h) pairs_job0 += x;
    const std::string path = std::string(dir) + "/pairs_" + (IS_G2 ? "g2" : "g1") + "_c" + std::to_string(c) + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return;
    const uint32_t head[6] = {c, n_mult, ext, job0.n, pairs_job0, job0.map ? 1u : 0u};
    fwrite(head, 4, 6, f);
    fwrite(sc.data(), 4, sc.size(), f);
    fwrite(mp.data(), 4, mp.size(), f);
    fclose(f);
}

// diagnostics: the heavy list of the set and the partials of its buckets
template <class HF, class DF>
void MsmGroup<HF, DF>::dump_heavy(const MsmPlan& p, hipStream_t st) {
    (void)hipStreamSynchronize(st);
    uint32_t nh = 0;
    (void)hipMemcpy(&nh, counter(p, N_HEAVY), 4, hipMemcpyDeviceToHost);
    std::vector<uint32_t> hl(nh), ch(p.n_buckets);
    if (nh) (void)hipMemcpy(hl.data(), heavy.as<uint32_t>(), nh * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(ch.data(), cnt.as<uint32_t>(), p.n_buckets * 4, hipMemcpyDeviceToHost);
    uint32_t mx = 0, le = 0;
    uint64_t sum = 0;
    for (uint32_t q = 0; q < nh; q++) {
        const uint32_t nt = (ch[hl[q]] + p.seg - 1) / p.seg;
        mx = std::max(mx, nt);
        le += nt <= p.medium_max;
        sum += nt;
    }
    fprintf(stderr, "[heavy] nj %zu nb %u seg %u merge_inline %u: %u listed buckets (%u with <= %u partials), %llu partials, largest %u\n", p.nj, nb,
            p.seg, p.merge_inline, nh, le, p.medium_max, (unsigned long long)sum, mx);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::copy_to_host(const DevBuf& stage, size_t n, typename MsmGroup<HF, DF>::HPoint* out, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, stage.p, n * sizeof(HPoint), hipMemcpyDeviceToHost, st));
    return ZK_OK;
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::normalize_to_host(const typename MsmGroup<HF, DF>::DPoint* src, size_t n, typename MsmGroup<HF, DF>::HPoint* out, DevBuf& stage, hipStream_t st) {
    if (!n) return ZK_OK;
    ZK_TRY(stage.ensure(n * sizeof(HPoint)));
    // a handful of points (a proof made alone): the Euclidean inversion, 0.66 -> 0.1 ms of pure latency; a chunk of
    // proofs: the Fermat chain, whose lanes stay in step (5.0 against 5.5 ms per 1024 proofs)
    if (n <= 64) {
        ZK_LAUNCH((zkdev::k_xyzz_normalize_export<DF, true>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, src,
                  stage.as<uint32_t>(), (uint32_t)n);
    } else {
        ZK_LAUNCH((zkdev::k_xyzz_normalize_export<DF, false>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, src,
                  stage.as<uint32_t>(), (uint32_t)n);
    }
    return copy_to_host(stage, n, out, st);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::export_to_host(const typename MsmGroup<HF, DF>::DPoint* src, size_t n, typename MsmGroup<HF, DF>::HPoint* out, DevBuf& stage, hipStream_t st) {
    if (!n) return ZK_OK;
    ZK_TRY(stage.ensure(n * sizeof(HPoint)));
    ZK_LAUNCH(zkdev::k_export_xyzz<DF>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, src, stage.as<uint32_t>(), (uint32_t)n);
    return copy_to_host(stage, n, out, st);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::normalize2_to_host(const typename MsmGroup<HF, DF>::DPoint* src0, const typename MsmGroup<HF, DF>::DPoint* src1, size_t n, typename MsmGroup<HF, DF>::HPoint* out0, typename MsmGroup<HF, DF>::HPoint* out1, DevBuf& stage0,
                                 DevBuf& stage1, hipStream_t st) {
    if (2 * n > 64) {
        ZK_TRY(normalize_to_host(src0, n, out0, stage0, st));
        return normalize_to_host(src1, n, out1, stage1, st);
    }
    if (!n) return ZK_OK;
    ZK_TRY(stage0.ensure(n * sizeof(HPoint)));
    ZK_TRY(stage1.ensure(n * sizeof(HPoint)));
    ZK_LAUNCH((zkdev::k_xyzz_normalize_export2<DF, true>), dim3(1), dim3(64), 0, st, src0, src1, stage0.as<uint32_t>(),
              stage1.as<uint32_t>(), (uint32_t)n);
    ZK_TRY(copy_to_host(stage0, n, out0, st));
    return copy_to_host(stage1, n, out1, st);
}

template <class HF, class DF>
zk_status MsmGroup<HF, DF>::run(std::vector<MsmJob>& jobs, std::vector<typename MsmGroup<HF, DF>::HPoint>& out, const zkdev::MsmSelSet* sels) {
    ZK_TRY(enqueue(jobs, out, g_stream, true, sels));
    return collect(g_stream);
}

}  // namespace zkrt
