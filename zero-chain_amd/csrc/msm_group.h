// The MSM group (moved out of zkamd.cpp in round 6): the doubling table of a set of bases + the bucket pipeline over a list of
// jobs (sort, accumulation, bucket reduction), a class template over the host / device field pair.  It is instantiated twice
// - G1 on Fq28, G2 on Fq2x - and each instantiation compiles ~25 kernels (overview: msm.h), among them the generated assembly loops:
// msm_g1.cpp and msm_g2.cpp hold one explicit instantiation each (ZK_MSM_GROUP_INSTANTIATE), every other unit sees them as
// `extern template` and compiles none of their kernels - an edit of the prover's host logic no longer rebuilds them, and the
// three units compile side by side.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <utility>
#include <mutex>
#include "../../include/zkamd.h"
#include "gpu_rt.h"
#include "host_common.h"
#include "host_math.h"
#include "msm_types.h"
#include "coop_tail.h"
#include "msm_plan.h"

namespace zkrt {

// Width of the NAF recoding for jobs of about n scalars: minimise, in units of one mixed addition,
//   n * 254 / (c + 1)  (bucket accumulation)  +  beta * 2^(c-2)  (bucket reduction),
// beta = measured cost of reducing one bucket relative to one mixed addition of the same group
// (G1: 2-3 full additions of 14 products against a mixed addition of 10, plus the tree above;
// G2: the same in Fq2, where the full addition no longer fits the register file).  `group` 1 / 2.
// group: 1 = G1 jobs of a batch (level 1 of their reduction in assembly), 2 = G2, 3 = the small A jobs of a split batch,
// 4 = a stand-alone G1 handle (zk_msm_create: compiled reduction)
// Over a table with multiples (msm_types.h MsmRecode) a scalar has 254 / (c + 1 + g) digits, g = 0.6 / 1.25 / 1.85 bits for 2 / 4 / 8
// multiples; the widths are NOT taken from that: with it the G2 set came out at 12 and ran 3.4 ms per chunk slower than at the
// 13 it has without (profiles/r28_table_multiples.txt (c)), so the bound sets keep the widths of one multiple.
inline uint32_t pick_window(size_t n, int group) {
    const char* env = getenv(group == 2 ? "ZKAMD_WINDOW_BITS_G2" : group == 3 ? "ZKAMD_WINDOW_BITS_G1A" : "ZKAMD_WINDOW_BITS_G1");
    if (!env) env = getenv("ZKAMD_WINDOW_BITS");
    if (env && atoi(env) >= 2 && atoi(env) <= 22) return (uint32_t)atoi(env);
    const char* benv = getenv(group == 2 ? "ZKAMD_BUCKET_COST_G2" : "ZKAMD_BUCKET_COST_G1");
    // G1: 2.2 full additions of ~6 100 instructions per bucket in the assembly loop of level 1 plus the compiled levels
    // above it, against 4 324 per mixed addition (round 3, compiled level 1: 6)
    // (group 3, the small A jobs of a split batch: their reduction is half latency - the levels above the assembly loop -
    //  so a bucket weighs more; 14 and 15 measured the same, profiles/r04_experiments.txt r04g: the narrower one it is)
    const double beta = benv && atof(benv) > 0 ? atof(benv) : (group == 2 ? 12.0 : group == 1 ? 4.0 : 6.0);
    uint32_t best = 2;
    double best_cost = 1e300;
    for (uint32_t c = 2; c <= 22; c++) {
        double cost = 254.0 / (c + 1) * (double)(n ? n : 1) + beta * (double)((size_t)1 << (c - 2));
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// On-curve + subgroup validation of an array of decoded points (Parameters::read(checked = true):
// core/pairing/src/bls12_381/ec.rs:675-688), one GPU thread per point.
template <class HF, class DF>
zk_status check_points_dev(const zkdev::Affine<DF>* d_pts, size_t n, const char* what);
template <class HF, class DF>
zk_status check_points_host(const std::vector<zkhost::Affine<HF>>& pts, const char* what);
// The other point kernels two units need, behind host functions (DF = zkdev::Fq or DevFq2; all four are defined in
// msm_group_impl.h and instantiated by msm_g1.cpp / msm_g2.cpp, where alone their kernels are compiled):
// dst[i] = the host-layout affine point i of d_src, n points, enqueued on st
template <class DF>
zk_status import_affine_dev(const void* d_src, zkdev::Affine<DF>* dst, size_t n, hipStream_t st);
// the doublings - and, behind them, those of the odd multiples j0 <= j < n_mult - of the n points in slice 0 of `table`,
// npos slices each, enqueued on st; `scratch` is sized here and must outlive the launch
template <class DF>
zk_status build_table_dev(zkdev::Affine<DF>* table, size_t n, uint32_t npos, DevBuf& scratch, uint32_t n_mult, uint32_t j0, hipStream_t st);

// Which form of the two scratch-using assembly kernels a device runs (msm_asm_g2.h: the G2 accumulation loop; msm_asm_g1.h:
// level 1 of the G1 reduction; 0 = the first form, 84 - 144 B of scratch per lane; 1 = the scratch-free second form).  Decided per device
// when the first key is loaded there (calibrate_kernel_forms below); ZKAMD_KERNEL_FORM = scratch | free overrides.
struct KernelForms {
    bool done = false;
    uint32_t form[2] = {0, 0};          // [G2 accumulation, G1 reduction level 1]
    float ms[4] = {0, 0, 0, 0};         // the comparison: [G2 first form, G2 scratch-free, reduction first form, reduction scratch-free]
};
inline std::mutex g_forms_mu;
inline KernelForms g_forms[64];
inline uint32_t kernel_form(int which) {
    static const int forced = [] {
        const char* e = getenv("ZKAMD_KERNEL_FORM");
        return !e ? -1 : !strcmp(e, "free") ? 1 : !strcmp(e, "scratch") ? 0 : -1;
    }();
    if (forced >= 0) return (uint32_t)forced;
    return g_forms[g_device & 63].form[which];   // (written once, before the device's first proving launch)
}

// The accumulation kernels run the generated assembly loops (msm_asm_g1.h k_msm_accumulate_g1asm / msm_asm_g2.h _g2asm) from
// ZKAMD_ASM_MIN_PAIRS pairs per launch set on, unless the build has none (the x86 emulation build).
template <class DF>
constexpr bool asm_loop() { return false; }
template <class DF>
void launch_asm_loop(const zkdev::Affine<DF>*, const uint32_t*, const uint4*, const uint32_t*, zkdev::XYZZ<DF>*, uint32_t*,
                            uint32_t*, unsigned, hipStream_t) {}
// Level 1 of the bucket reduction as the generated assembly loop (msm_asm_g1.h k_msm_reduce1_g1asm): G1 only, unless
// the build has none (the x86 emulation build).
template <class DF>
constexpr bool asm_reduce() { return false; }
template <class DF>
void launch_red_asm(const zkdev::XYZZ<DF>*, const uint32_t*, const uint32_t*, const uint32_t*, zkdev::XYZZ<DF>*, zkdev::XYZZ<DF>*,
                           uint32_t, uint32_t, dim3, hipStream_t, uint32_t*, uint32_t*) {}
// (the launchers' definitions: msm_g1.cpp / msm_g2.cpp, next to the generated assembly kernels they launch)
#ifdef ZK_HAVE_RED_ASM
template <> constexpr bool asm_reduce<zkdev::Fq28>() { return true; }
template <>
void launch_red_asm<zkdev::Fq28>(const zkdev::XYZZ<zkdev::Fq28>* tsums, const uint32_t* cnt, const uint32_t* toff, const uint32_t* tbase,
                                 zkdev::XYZZ<zkdev::Fq28>* S, zkdev::XYZZ<zkdev::Fq28>* A, uint32_t nb, uint32_t L, dim3 grid,
                                 hipStream_t st, uint32_t* n_fallback, uint32_t* fallback);
#endif
#ifdef ZK_HAVE_MADD_ASM
int persist_wgs(int group = 1);
template <> constexpr bool asm_loop<zkdev::Fq28>() { return true; }
template <> constexpr bool asm_loop<zkdev::Fq2x>() { return true; }
template <>
void launch_asm_loop<zkdev::Fq28>(const zkdev::Affine<zkdev::Fq28>* table, const uint32_t* pairs, const uint4* sorted,
                                  const uint32_t* d_total, zkdev::XYZZ<zkdev::Fq28>* tsums, uint32_t* d_nredo, uint32_t* redo,
                                  unsigned blocks, hipStream_t st);
template <>
void launch_asm_loop<zkdev::Fq2x>(const zkdev::Affine<zkdev::Fq2x>* table, const uint32_t* pairs, const uint4* sorted,
                                  const uint32_t* d_total, zkdev::XYZZ<zkdev::Fq2x>* tsums, uint32_t* d_nredo, uint32_t* redo,
                                  unsigned blocks, hipStream_t st);
#endif

// The sort and the task order of a launch set do not depend on the group: plain functions over the plan of the set and the
// pointers of the group's workspaces, defined in msm_g1.cpp next to the kernels they launch (msm_sort.h), called by both groups.
struct MsmSortBufs {
    const MsmJob* jobs;
    uint32_t *cnt, *off, *toff, *ntasks, *pairs, *blockbase, *coarse;
    uint2* rank;
    uint32_t *hist, *tclass, *tbase;   // hist: [length histogram | cursors] of the task order (msm_plan.h Bytes::hist)
    uint4* sorted;
    uint32_t *heavy, *light;           // light: null where the set lists no light buckets
    uint32_t *n_tasks, *n_heavy, *n_light;
};
// the (digit, point) pairs of every job sorted by bucket: cnt / off of every bucket, toff = its first task
zk_status msm_sort_pairs(const MsmPlan& p, hipStream_t st, const MsmSortBufs& w, uint32_t nb, uint32_t c, const zkdev::MsmRecode& rc,
                         const zkdev::MsmSelSet& sel_set);
// the tasks of the set in classes of equal length, longest first (`sorted`), and the heavy / light lists of the merge
zk_status msm_order_tasks(const MsmPlan& p, hipStream_t st, const MsmSortBufs& w, uint32_t nb);

template <class HF, class DF>
struct MsmGroup {
    typedef zkhost::Affine<HF> HAffine;
    typedef zkhost::Point<HF> HPoint;
    typedef zkdev::Affine<DF> DAffine;
    typedef zkdev::XYZZ<DF> DPoint;
    // host layout = the reference's (6 x u64 Montgomery limbs per Fq); the device keeps G1 in
    // radix-2^28 limbs: k_import_affine / k_export_xyzz convert at the two ends of a run
    static_assert(sizeof(HAffine) == 2 * 4 * zkdev::HostWords<DF>::N, "host affine layout");
    static_assert(sizeof(HPoint) == 4 * 4 * zkdev::HostWords<DF>::N, "host point layout");

    static constexpr bool IS_G2 = zkdev::HostWords<DF>::N == 24;

    uint32_t c = 0, maxd = 0, nb = 0;
    size_t n_points = 0;
    // the odd multiples of every slice the table holds (msm_types.h MsmRecode; 1: the doublings alone), the extra window bits of the
    // recoding over them and its choice table for this group's c (made by the first launch set: ensure_recode)
    uint32_t n_mult = 1, ext = 0;
    DevBuf table, lut;
    DevBuf jobs_d, cnt, off, toff, ntasks, hist, tclass, sorted, heavy, light, blockbase, coarse, tbase, rank, pairs, tsums, red_r, red_w, red_t, result, redo;
    DPoint* res_dev = nullptr;
    PinBuf pin_jobs;
    size_t bytes = 0;
    DevBuf dstat;   // [first refused encoding | points at infinity] of the last decode_enqueue (msm_point_kernels.h k_decode_uncompressed)

    // the recoding width and what follows from it.  with_table = false: variable-base mode - only the bases themselves are
    // kept (slice 0), every job takes ONE digit of every scalar (msm_recode.h msm_digits)
    zk_status set_geometry(uint32_t c_, size_t n, bool with_table, uint32_t n_mult_ = 1) {
        if (n_mult_ < 1 || n_mult_ > zkdev::MSM_MULT_MAX || (n_mult_ > 1 && !with_table))
            return fail(ZK_ERR_INVALID_ARGUMENT, "internal: table multiples out of range");
        c = c_;
        maxd = with_table ? zkdev::msm_max_digits(c) : 1u;
        nb = 1u << (c - 2);
        n_points = n;
        set_multiples(n_mult_);
        const uint32_t npos = with_table ? zkdev::MSM_NPOS : 1u;
        // a pair is an entry's index and a sign bit: 31 bits for the index
        if ((uint64_t)n_points * npos * n_mult >= (1ull << 31)) return fail(ZK_ERR_INVALID_ARGUMENT, "doubling table too large");
        bytes = sizeof(DAffine) * n_points * npos * n_mult;
        return ZK_OK;
    }
    // the same bases (borrowed doubling table, with its multiples) under another recoding width; workspaces are this object's own
    void alias(const MsmGroup& o, uint32_t c_) {
        (void)set_geometry(c_, o.n_points, true, o.n_mult);   // (the table it borrows passed the size test when it was built)
        bytes = 0;                                              // (... and is accounted for by its owner)
        table.borrow(o.table);
    }
    void set_multiples(uint32_t n_mult_) {
        n_mult = n_mult_;
        ext = zkdev::msm_mult_ext(n_mult);
        if (c + ext > 22) ext = c < 22 ? 22 - c : 0;   // (the recoding's buffer holds 32 bits: msm_recode.h msm_wnaf_mult)
        lut.release();
    }
    // A table built with one multiple gets the slices of the others: a new allocation, the slices in place copied, the chains of
    // 3 P, 5 P, ... made (a key bound by a proof made alone meets its first batch).  Groups that borrowed the table alias again.
    zk_status add_multiples(uint32_t n_mult_);
    // the choice table of the recoding over the multiples (none for one multiple), and what the sort kernels get
    zk_status ensure_recode();
    zkdev::MsmRecode recode() const { return zkdev::MsmRecode{lut.as<uint8_t>(), n_mult, ext}; }
    // Slice 0 of the table from the reference's uncompressed encodings (n x 96 / 192 bytes on the HOST), decoded on the
    // device: upload into `raw`, k_decode_uncompressed into the table, `map` (n entries) = position or -1 for a point at
    // infinity.  Everything is enqueued on st; decode_finish() reads the verdict once the stream has been waited for.
    zk_status decode_enqueue(const uint8_t* bases, size_t n, uint32_t c_, bool with_table, DevBuf& raw, DevBuf& map, hipStream_t st);
    // after the stream was waited for: ZK_ERR_IO naming the first refused encoding, else *n_inf = points at infinity
    // (*bad_index = the refused encoding's index when the status is ZK_ERR_IO for that reason; a device error leaves it alone)
    zk_status decode_finish(const char* what, uint32_t* n_inf, size_t* bad_index = nullptr) {
        uint32_t v[2] = {0xffffffffu, 0};
        HIP_TRY(hipMemcpy(v, dstat.p, 8, hipMemcpyDeviceToHost));
        if (v[0] != 0xffffffffu) {
            if (bad_index) *bad_index = v[0];
            return fail(ZK_ERR_IO, std::string("invalid ") + (IS_G2 ? "G2" : "G1") + " encoding at " + what + " " + std::to_string(v[0]));
        }
        *n_inf = v[1];
        return ZK_OK;
    }
    // the table of doublings over a slice 0 that is in place, enqueued on st (the caller waits and then frees `scratch`)
    zk_status table_enqueue(DevBuf& scratch, hipStream_t st);
    // the table of doublings over a slice 0 that is already in place; checked: curve + subgroup test of every base first
    zk_status finish_build(bool checked, const char* what, bool with_table);
    zk_status build(const std::vector<HAffine>& pts, uint32_t c_, bool checked, const char* what, bool with_table = true,
                    uint32_t n_mult_ = 1);

    // A derived base set: slice 0 = [pts | entries [from, from + count) of slice 0 of `o`], then the table of doublings.  A point
    // at infinity among pts stays (0, 0) through the table, as in a key file: the caller maps it out.
    zk_status build_with_tail(const std::vector<HAffine>& pts, const MsmGroup& o, size_t from, size_t count, uint32_t c_,
                              uint32_t n_mult_ = 1);

    // jobs[i].pair_base is filled in here.  Everything, including the copy of the results (one XYZZ
    // per job) into `out`, is enqueued on `st`; collect() waits for it.
    // sels: the pair slots of the set's jobs whose bases follow the bytes of this call's proofs (msm_types.h MsmSelSet), or null.
    zk_status enqueue(std::vector<MsmJob>& jobs, std::vector<HPoint>& out, hipStream_t st, bool to_host = true,
                      const zkdev::MsmSelSet* sels = nullptr);
    // out[i] = affine form of src[i] (host layout, zz = zzz = 1), enqueued on st
    zk_status normalize_to_host(const DPoint* src, size_t n, HPoint* out, DevBuf& stage, hipStream_t st);
    // out[i] = src[i] as it is (host layout, zz and zzz NOT normalised: zkhost::to_affine inverts), enqueued on st.  For a
    // handful of proofs made alone: three inversions on a host core are 0.1 ms, the two normalisation kernels 0.3 - 0.37 ms
    // each on the critical path of a 2.4 ms proof (profiles/r06e_*).
    zk_status export_to_host(const DPoint* src, size_t n, HPoint* out, DevBuf& stage, hipStream_t st);
    // two arrays of n points each, out0 / out1 on the host; one launch while the pair fits a wave
    zk_status normalize2_to_host(const DPoint* src0, const DPoint* src1, size_t n, HPoint* out0, HPoint* out1, DevBuf& stage0,
                                 DevBuf& stage1, hipStream_t st);
    zk_status collect(hipStream_t st) {
        HIP_TRY(hipStreamSynchronize(st));
        return ZK_OK;
    }
    zk_status run(std::vector<MsmJob>& jobs, std::vector<HPoint>& out, const zkdev::MsmSelSet* sels = nullptr);
    // The (digit, point) pairs of the last launch set, nj jobs, counted from its buckets; after collect() and before the next
    // enqueue on this group.  For measurements (ZKAMD_TRACE_HOST): it reads nj * nb words back.
    zk_status count_pairs(size_t nj, uint64_t* total) {
        std::vector<uint32_t> h(nj * (size_t)nb);
        *total = 0;
        if (h.empty() || !cnt.p) return ZK_OK;
        HIP_TRY(hipMemcpy(h.data(), cnt.p, h.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t x : h) *total += x;
        return ZK_OK;
    }

private:
    // the table of doublings over slice 0, enqueued on st
    zk_status launch_table_build(DevBuf& scratch, hipStream_t st);
    // the stages of enqueue(), in its order, each over the plan of the set (msm_plan.h)
    zk_status reserve(const MsmPlan& p, bool to_host);
    zk_status upload_jobs(const std::vector<MsmJob>& jobs, const MsmPlan& p, hipStream_t st);
    zk_status sort_pairs(const MsmPlan& p, hipStream_t st, const zkdev::MsmSelSet& sel_set);
    zk_status order_tasks(const MsmPlan& p, hipStream_t st);
    MsmSortBufs sort_bufs(const MsmPlan& p) const {
        return MsmSortBufs{jobs_d.as<MsmJob>(), cnt.as<uint32_t>(), off.as<uint32_t>(), toff.as<uint32_t>(), ntasks.as<uint32_t>(),
                           pairs.as<uint32_t>(), blockbase.as<uint32_t>(), coarse.as<uint32_t>(), rank.as<uint2>(), hist.as<uint32_t>(),
                           tclass.as<uint32_t>(), tbase.as<uint32_t>(), sorted.as<uint4>(), heavy.as<uint32_t>(),
                           p.use_light ? light.as<uint32_t>() : nullptr, counter(p, N_TASKS), counter(p, N_HEAVY), counter(p, N_LIGHT)};
    }
    zk_status accumulate(const MsmPlan& p, hipStream_t st);
    zk_status merge_partials(const MsmPlan& p, hipStream_t st);
    zk_status level1(const MsmPlan& p, hipStream_t st);
    zk_status tail(const MsmPlan& p, hipStream_t st);
    // the end of the *_to_host functions: the launch is checked, `stage` (n points in the host's layout) goes to `out`
    zk_status copy_to_host(const DevBuf& stage, size_t n, HPoint* out, hipStream_t st);
    // diagnostics of the hooks build (ZKAMD_DEBUG_REDO, ZKAMD_DEBUG_HEAVY, ZKAMD_DEBUG_PAIRS)
    void dump_pairs(const MsmJob& job0, hipStream_t st, const char* dir);
    void dump_redo(const MsmPlan& p, hipStream_t st, bool after_level1);
    void dump_heavy(const MsmPlan& p, hipStream_t st);
    // the counters behind the two class arrays of `hist` (its layout: msm_plan.h Bytes::hist)
    enum Counter { N_TASKS = 0, N_HEAVY = 1, N_REDO = 2, N_LIGHT = 4, N_FALLBACK = 5 };
    uint32_t* counter(const MsmPlan& p, Counter k) const { return hist.as<uint32_t>() + 2 * p.n_class + k; }
    DPoint* node_s() const { return red_r.as<DPoint>(); }   // S of the nodes of level 1: node t of job j at [(j T + t) s_stride]
    DPoint* node_w() const { return red_w.as<DPoint>(); }   // W of the nodes, compact
    DPoint* job_sums(const MsmPlan& p) const { return node_w() + p.nj * (size_t)p.T; }   // one XYZZ per job
};

typedef MsmGroup<zkhost::Fq, zkdev::Fq> MsmG1;
// G2 runs on Fq2 over the radix-2^28 representation with the fused lazy-reduction product (dev_field.h Fq2x)
typedef zkdev::Fq2x DevFq2;
typedef MsmGroup<zkhost::Fq2, DevFq2> MsmG2;
typedef zkhost::Affine<zkhost::Fq> HG1A;
typedef zkhost::Affine<zkhost::Fq2> HG2A;
typedef zkhost::Point<zkhost::Fq> HG1;
typedef zkhost::Point<zkhost::Fq2> HG2;

// the load-time comparison of the two forms of the scratch-using assembly kernels (zkamd.cpp calibrate_kernel_forms): each
// half next to the kernels it launches.  ms[0] = the first form, ms[1] = the scratch-free form, best of two counted runs.
zk_status calibrate_g2_accumulate(const zkdev::Affine<DevFq2>* table, uint32_t n_entries, float ms[2]);
zk_status calibrate_g1_reduce(const zkdev::Affine<zkdev::Fq28>* table, uint32_t n_entries, float ms[2]);

#ifndef ZK_MSM_GROUP_INSTANTIATE
extern template struct MsmGroup<zkhost::Fq, zkdev::Fq>;
extern template struct MsmGroup<zkhost::Fq2, DevFq2>;
#endif
// (msm_g1.cpp / msm_g2.cpp: the group and the four point functions above, over the unit's field)
#define ZK_MSM_GROUP_DEFINE(HF, DF)                                                                                         \
    template struct MsmGroup<HF, DF>;                                                                                       \
    template zk_status check_points_dev<HF, DF>(const zkdev::Affine<DF>*, size_t, const char*);                             \
    template zk_status check_points_host<HF, DF>(const std::vector<zkhost::Affine<HF>>&, const char*);                      \
    template zk_status import_affine_dev<DF>(const void*, zkdev::Affine<DF>*, size_t, hipStream_t);                         \
    template zk_status build_table_dev<DF>(zkdev::Affine<DF>*, size_t, uint32_t, DevBuf&, uint32_t, uint32_t, hipStream_t);

}  // namespace zkrt
