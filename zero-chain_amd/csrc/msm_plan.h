// The plan of one MSM launch set (msm_group.h MsmGroup::enqueue): every decision about its shape and the size of every
// workspace it reserves, as pure integer arithmetic on (group, window, the jobs' sizes, the tunables) - nothing here touches
// the HIP runtime, so the CPU suite pins the plans of the product's launch sets (tests/test_msm_plan.py, through
// zk_hook_msm_plan).  A threshold that moves by accident still gives correct proofs - the bytes do not depend on the
// order of summation - which is why it is pinned here and not only through proof bytes.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../include/zkamd.h"
#include "msm_types.h"
#include "coop_tail.h"

namespace zkrt {

using zkdev::MsmJob;

// At most this many jobs per launch set: the latency-optimised form (many-workgroup sort, bit-plane tail of the bucket
// reduction: coop_tail.h planes / combine).  8 until round 5; a kernel trace of a 32-proof call then showed the many-jobs form's eleven k_msm_segsum<Fq2x>
// launches - 0.8 ms each whether for 32 jobs or 1024: 8.9 of the call's 16.8 ms - and the sweep of tools/few_jobs_probe.py
// (profiles/r05end_few_jobs_probe.txt, same proof bytes under every setting): 8 proofs per call 10.5 -> 7.8 ms, 16: 14.9 -> 10.9,
// 32: 19.9 -> 17.6, 64: 35.1 -> 30.1, 128: 51.6 -> 49.7; from 256 jobs on the many-jobs form wins (86.1 against 90.2).
constexpr size_t MSM_FEW_JOBS = 128;
constexpr uint32_t MSM_RED_FAN = 16;   // buckets per level-1 node and children per upper node (bucket reduction)

// The environment variables a launch set reads, each with its own parsing rule: overrides for measurements and for the
// tests.  Read at every launch set and in this one place (the emulation suite flips them between calls: nothing is static).
struct MsmTunables {
    uint32_t seg_forced;        // ZKAMD_MSM_SEG (G2: ZKAMD_MSM_SEG_G2 first): points per accumulation task; 0 = not forced
    size_t few_jobs_max;        // ZKAMD_FEW_JOBS
    uint64_t coop_l1_max;       // ZKAMD_COOP_L1_MAX
    uint64_t asm_min_pairs;     // ZKAMD_ASM_MIN_PAIRS
    bool no_lds_sort;           // ZKAMD_NO_LDS_SORT
    uint32_t sort_fine_log;     // ZKAMD_SORT_FINE_LOG
    uint32_t merge_split_min;   // ZKAMD_MERGE_SPLIT_MIN (read by coop_tail.cpp, whose kernels take it too)

    static MsmTunables read(bool is_g2) {
        MsmTunables t;
        // (a segment size outside 1 .. MSM_SEG_MAX is ignored)
        const char* seg_env = getenv(is_g2 && getenv("ZKAMD_MSM_SEG_G2") ? "ZKAMD_MSM_SEG_G2" : "ZKAMD_MSM_SEG");
        t.seg_forced = seg_env && atoi(seg_env) > 0 && atoi(seg_env) <= (int)zkdev::MSM_SEG_MAX ? (uint32_t)atoi(seg_env) : 0u;
        const char* few_env = getenv("ZKAMD_FEW_JOBS");
        t.few_jobs_max = few_env && atoll(few_env) > 0 ? (size_t)atoll(few_env) : MSM_FEW_JOBS;
        // (G2: 16 384 - an addition on a row is 2.4 x G1's, and the 80 k buckets of the 2^17-point variable-base G2 multiexp took
        //  1.73 ms for merge + level 1 on rows against 0.8 ms with the lanes' kernels and only the heavy buckets on rows)
        const char* l1_env = getenv("ZKAMD_COOP_L1_MAX");
        t.coop_l1_max = l1_env ? (uint64_t)atoll(l1_env) : (is_g2 ? 16384ull : 131072ull);
        // launches large enough for the assembly loops (accumulation and level 1 of the reduction); tests set 0: every
        // launch, however small, goes through them
        // (G2 additions are three times as long: its loop pays from a quarter of the pairs - the 2^17-point variable-base G2
        //  multiexp, 2.5 M pairs: accumulation 1.89 -> 1.37 ms, profiles/r06z_*)
        const char* min_env = getenv("ZKAMD_ASM_MIN_PAIRS");
        t.asm_min_pairs = min_env ? (uint64_t)atoll(min_env) : (is_g2 ? 1000000ull : 4000000ull);
        t.no_lds_sort = getenv("ZKAMD_NO_LDS_SORT") != nullptr;
        const char* fine_env = getenv("ZKAMD_SORT_FINE_LOG");
        t.sort_fine_log = fine_env ? (uint32_t)atoi(fine_env) : 7u;
        t.merge_split_min = zkcoop::merge_split_min();
        return t;
    }
};

struct MsmPlan {
    zk_status status = ZK_OK;
    const char* refusal = nullptr;     // the message of a status other than ZK_OK
    bool is_g2 = false;
    uint32_t c = 0, nb = 0;
    size_t nj = 0;
    uint32_t max_n = 0;                // the longest job
    uint64_t total = 0;                // (digit, point) pairs of the set
    uint64_t total_tasks = 0;          // upper bound on its accumulation tasks
    size_t n_buckets = 0, n_class = 0;
    std::vector<uint32_t> pair_base;   // per job: its first slot in the rank / pair arrays
    std::vector<uint32_t> tbase;       // per job: its first task
    uint32_t seg = 0;                  // points per accumulation task
    bool few = false;                  // the latency-optimised form of the set
    bool coop_l1 = false;              // merge and level 1 on rows
    uint32_t coop_rb = 1;              // rows per bucket of the cooperative merge
    uint32_t merge_inline = 0;         // buckets with more task partials go onto the heavy list
    size_t heavy_cap = 0, light_cap = 0;
    bool use_light = false;            // buckets with 2 .. merge_inline partials are listed for k_msm_merge_light
    uint32_t heavy_blocks = 0;
    uint32_t medium_max = 0;           // (MEDIUM_MAX of the merge on lanes)
    bool big_launch = false;
    bool acc_asm = false, red_asm = false;   // the assembly loops: accumulation, level 1 of the reduction
    uint32_t L = 0, T = 0;             // buckets per node of level 1, nodes per job
    uint32_t nbits = 0, log2_2l = 1;   // log2(T), log2(2 L)
    uint32_t s_stride = 0;
    uint32_t nsplit = 0;               // workgroups per bit plane (coop_tail.h planes)
    bool lds_sort = false;
    uint32_t fine_log = 0, n_coarse = 0, coarse_wgs = 0;   // the two-level counting sort (0 with the LDS sort)
    struct Bytes {                     // the workspaces of the set (0: not reserved)
        size_t jobs_d, bucket /* cnt, off, toff */, per_job /* ntasks, tbase */, hist, heavy, light, tclass, sorted, tsums, pairs, red_r,
            red_w, red_t, pin_jobs, rank, blockbase, coarse, redo, result /* reserved when the results go to the host */;
    } bytes = {};

    zk_status refuse(const char* why) {
        status = ZK_ERR_INVALID_ARGUMENT;
        refusal = why;
        return status;
    }
};

// `maxd`: digits per scalar a job takes (1 in variable-base mode); has_asm_loop / has_asm_reduce: whether the build has the
// generated assembly loop of the accumulation / of level 1 for this group (msm_group.h asm_loop, asm_reduce)
inline zk_status msm_plan(MsmPlan& p, bool is_g2, uint32_t c, uint32_t nb, uint32_t maxd, const MsmJob* jobs, size_t nj, bool has_asm_loop,
                          bool has_asm_reduce, const MsmTunables& tun) {
    const size_t point = is_g2 ? sizeof(zkdev::XYZZ<zkdev::Fq2x>) : sizeof(zkdev::XYZZ<zkdev::Fq28>);
    p = MsmPlan();
    p.is_g2 = is_g2;
    p.c = c;
    p.nb = nb;
    p.nj = nj;
    uint64_t total = 0, total_tasks = 0;
    for (size_t k = 0; k < nj; k++) total += (uint64_t)jobs[k].n * maxd;
    // points per accumulation task (msm_accumulate.h): a task is a serial chain of ~10 us per point, so the
    // long form is for launches that keep the GPU busy for tens of milliseconds anyway
    // ... and the short form (32) is for one proof at a time, where the longest task IS the launch: 5.33 -> 4.80 ms
    // per proof (at 2^20 points it costs 1 % with the table and doubles the variable-base time: kept at 64 there)
    // (G2, whose additions take three times as long and whose side stream is the critical path of a lone proof: 16,
    // 3.79 -> 3.53 ms)
    const uint32_t seg = tun.seg_forced ? tun.seg_forced
                                        : (nj >= 64 && total >= 100000000ull ? 256u : total < 4000000ull ? (is_g2 ? 16u : 32u) : 64u);
    p.seg = seg;
    p.pair_base.resize(nj);
    p.tbase.resize(nj);
    total = 0;
    for (size_t k = 0; k < nj; k++) {
        p.pair_base[k] = (uint32_t)total;
        total += (uint64_t)jobs[k].n * maxd;
        p.max_n = std::max(p.max_n, jobs[k].n);
        // a bucket with k points becomes ceil(k / MSM_SEG) tasks: at most nb + pairs / SEG of them
        uint64_t cap = (uint64_t)nb + ((uint64_t)jobs[k].n * maxd) / seg + 1;
        p.tbase[k] = (uint32_t)total_tasks;
        total_tasks += cap;
    }
    p.total = total;
    p.total_tasks = total_tasks;
    if (total >= (1ull << 32) || total_tasks >= (1ull << 32)) return p.refuse("too many (digit, point) pairs in one launch");
    p.n_buckets = nj * (size_t)nb;
    if (p.n_buckets >= (1ull << 32)) return p.refuse("too many buckets in one launch");
    p.n_class = nj * (size_t)seg;
    // the latency-optimised form of the launch set (many-workgroup sort, bit-plane tail of the bucket reduction: msm_sort.h
    // passes 1-3, msm_reduce.h pass 5c, coop_tail.h planes / combine): one or a few jobs - and the digit positions of ONE variable-base
    // multiexp, a dozen or two jobs over the same large scalar vector, which are as far from filling the machine per job
    // as a lone job is.  Every other set is a chunk of proofs, which folds what is above level 1 on rows too, one
    // workgroup per job (coop_tail.h upper).
    const bool few = nj <= tun.few_jobs_max || jobs[0].vb_digit != 0;
    p.few = few;
    // A few jobs take merge and level 1 on rows as well while the buckets of the set are few enough for rows to be the right
    // grain: a row-addition is 4 - 5 x shorter than a lane's but a wave holds four rows instead of sixty-four lanes, so a set
    // of 278 528 buckets (the seventeen digit positions of a 2^20-point variable-base multiexp) keeps the lanes' kernels for
    // these two steps and goes onto rows where the reduction gets narrow (msm_reduce_g1 1.33 ms on lanes, 1.23 all on rows,
    // profiles/r06m_*)
    // (the bound and its G2 value: MsmTunables::read)
    const bool coop_l1 = few && (uint64_t)nj * nb <= tun.coop_l1_max;
    p.coop_l1 = coop_l1;
    // rows per bucket of the cooperative merge: a power of two near a quarter of the average number of partials
    uint32_t coop_rb = 1;
    if (coop_l1) {
        uint64_t est_tasks = (uint64_t)nj * nb;
        for (size_t k = 0; k < nj; k++) est_tasks += (uint64_t)jobs[k].n * maxd / seg;
        const uint64_t avg = est_tasks / ((uint64_t)nj * nb);
        while (coop_rb < 16 && coop_rb * 4 < avg) coop_rb <<= 1;
        // ... as long as the rows of the launch stay within ~2 waves per SIMD: beyond that the rows wait for each other's issue
        // slots and one row per bucket is the faster merge (the 2^17-point G2 multiexp, 19 456 buckets of ~8 partials: 1.47 ms
        // with four rows per bucket, profiles/r06o_vb_g2_launch_list.txt)
        while (coop_rb > 1 && (uint64_t)nj * nb * coop_rb > 16384) coop_rb >>= 1;
    }
    p.coop_rb = coop_rb;
    p.merge_inline = coop_l1 ? 8u * coop_rb : (nj >= 64 || few ? 8u : 2u);
    p.heavy_cap = (size_t)(total / ((size_t)seg * p.merge_inline)) + 1;
    p.heavy_blocks = (uint32_t)std::min<size_t>(p.heavy_cap, few ? 512 : 4096);
    // buckets with 2 .. merge_inline task partials (each holds more than seg pairs): listed for k_msm_merge_light
    p.use_light = !few;
    p.light_cap = (size_t)(total / seg) + 1;
    // (MEDIUM_MAX: never beyond the threshold from which the split form of coop_tail.cpp takes a bucket - a test lowers
    //  that one)
    p.medium_max = std::min<uint32_t>(64u, tun.merge_split_min);
    // level 1 on lanes: nodes of 16 buckets when that still leaves the machine full of threads, narrower nodes (a
    // shorter serial chain per thread) when one or a few jobs must fill it alone
    auto pick_fan = [&](uint64_t items) -> uint32_t {
        uint32_t f = MSM_RED_FAN;
        while (f > 4 && items / f < 32768) f >>= 1;
        return f;
    };
    // launches large enough for the assembly loops (the threshold: MsmTunables::read).  The accumulation: the assembly
    // loops are built for launches that fill the machine; a proof made alone (one or two jobs, 16- or 32-point tasks:
    // `total` below the short-task threshold above) keeps the compiled kernel and saves the second launch
    p.big_launch = total >= tun.asm_min_pairs;
    p.acc_asm = has_asm_loop && p.big_launch;
    // level 1 of the reduction in assembly: many-jobs launches only (the few-jobs tail folds level 1 differently)
    const bool red_asm = has_asm_reduce && p.big_launch && !few;
    p.red_asm = red_asm;
    // buckets per node of level 1 (a power of two).  The assembly loop: 32 - half the nodes for the tail above it, still
    // eight generations of waves per launch (16 / 32 / 64 measured within noise, r04g)
    const uint32_t L = std::min(nb, coop_l1 ? zkcoop::LEVEL1_FAN : red_asm ? 32u : pick_fan((uint64_t)nj * nb));
    const uint32_t T = nb / L;
    p.L = L;
    p.T = T;
    while ((1u << p.nbits) < T) p.nbits++;
    while ((1u << (p.log2_2l - 1)) < L) p.log2_2l++;
    // level 1 on rows and in assembly leaves one S per node; on lanes S is the first of a node's L suffix sums
    p.s_stride = coop_l1 || red_asm ? 1u : L;
    // a few jobs: the parts of the planes when a plane takes several workgroups, then the planes' sums Y (coop_tail.h planes)
    p.nsplit = zkcoop::planes_split(T);
    // one workgroup per job sorts inside its LDS: right for a thousand jobs per launch, a 0.67 ms serial pass for
    // the one or two jobs of a proof made alone (4.83 -> 4.17 ms per proof with the many-workgroup sort instead)
    p.lds_sort = (size_t)nb * 4 <= 65536 && !few && !tun.no_lds_sort;
    MsmPlan::Bytes& b = p.bytes;
    if (!p.lds_sort) {
        // two-level counting sort, every per-digit atomic in LDS (msm_sort.h)
        uint32_t fine_log = tun.sort_fine_log;
        while (fine_log < c - 2 && (nb >> fine_log) > zkdev::MSM_COARSE_MAX) fine_log++;
        if (fine_log > c - 2) fine_log = c - 2;
        if ((1u << fine_log) > zkdev::MSM_FINE_MAX) return p.refuse("ZKAMD_SORT_FINE_LOG out of range");
        p.fine_log = fine_log;
        p.n_coarse = nb >> fine_log;
        p.coarse_wgs = std::max(1u, (p.max_n + zkdev::MSM_COARSE_SCALARS - 1) / zkdev::MSM_COARSE_SCALARS);
        b.rank = (size_t)(total ? total : 1) * sizeof(uint2);     // (bucket in bin, pair) records
        b.blockbase = (size_t)p.coarse_wgs * nj * p.n_coarse * 4;   // the range a workgroup reserved in every bin
        b.coarse = 4 * nj * (size_t)p.n_coarse * 4;                 // bin counts | offsets | tasks | first task
    }
    b.jobs_d = nj * sizeof(MsmJob);
    b.bucket = p.n_buckets * 4;
    b.per_job = nj * 4;
    b.hist = (2 * p.n_class + 6) * 4;     // [length histogram | placement cursors | total | #heavy | #redo | next task block | #light | #level-1 nodes recomputed]
    b.heavy = p.heavy_cap * 4;
    b.light = p.use_light ? p.light_cap * 4 : 0;
    b.tclass = p.n_class * 4;
    b.sorted = (size_t)total_tasks * sizeof(uint4);
    b.tsums = (size_t)total_tasks * point;
    b.pairs = (size_t)(total ? total : 1) * 4;
    b.red_r = nj * (size_t)T * p.s_stride * point;
    b.red_w = nj * ((size_t)T + 1) * point;   // W of the nodes (assembly level 1: A) | the sum of every job
    b.red_t = few ? nj * (size_t)(p.nbits + 1) * (p.nsplit > 1 ? p.nsplit + 1 : 1) * point : 0;
    b.pin_jobs = nj * (sizeof(MsmJob) + 4);
    // the tasks the accumulation's assembly loop flagged for its second pass, then - that pass is done with its list by
    // then - the nodes the assembly level 1 hands to the compiled addition
    b.redo = p.acc_asm || red_asm ? std::max((size_t)total_tasks, nj * (size_t)T) * 4 : 0;
    b.result = nj * 4 * 4 * (size_t)(is_g2 ? zkdev::HostWords<zkdev::Fq2x>::N : zkdev::HostWords<zkdev::Fq28>::N);   // a point in the host's layout per job
    return ZK_OK;
}

}  // namespace zkrt
