// Passes 1 to 4 of the multiexp (overview: msm.h): the (digit, point) pairs of every job counting-sorted by bucket - in one
// workgroup's LDS, or in two levels where the histogram does not fit - and the tasks of the launch set ordered by length.
// The kernels do not depend on the group: msm_g1.cpp compiles and launches them for both (msm_group.h msm_sort_pairs /
// msm_order_tasks).
#pragma once
#include "msm_recode.h"

namespace zkdev {

// Passes 1-3 for jobs whose bucket histogram does NOT fit LDS (one or a few large multiexps,
// c >= 17): a two-level counting sort that keeps every per-digit atomic in LDS.
//   coarse bin = bucket >> fine_log  (n_coarse <= 1024 bins of `fine` = 2^fine_log buckets)
//   1. k_msm_coarse_count    a workgroup histograms the digits of its 1024 scalars over the coarse
//                            bins in LDS and reserves a range per bin with ONE global atomic
//   2. k_msm_coarse_scan     exclusive scan of the bin totals (one workgroup per job)
//   3. k_msm_coarse_scatter  the same workgroups recode again and write (bucket inside the bin,
//                            pair) records into their ranges: the digits are now grouped by bin
//   4. k_msm_fine_sort       one workgroup per bin: LDS histogram of its `fine` buckets, scan,
//                            scatter of the pairs; writes cnt / off / bin-local toff
//   5. k_msm_task_offsets    scan of the bins' task counts, added to toff
// (The first version took one returning global atomic per digit - 13.4 M of them for 2^20 scalars,
// 0.63 ms at ~21 G atomics/s - and remembered the tickets for an atomic-free scatter: 1.2 ms for
// the three passes against the accumulation's 3.1 ms.)

static __global__ void __launch_bounds__(256)
k_msm_coarse_count(const MsmJob* __restrict__ jobs, uint32_t c, uint32_t fine_log, uint32_t n_coarse, uint32_t* coarse_cnt,
                   uint32_t* blockbase, uint32_t per_wg, const MsmSelSet sels = MsmSelSet{}, const MsmRecode rc = MsmRecode{}) {
    ZK_SHARED uint32_t h[MSM_COARSE_MAX];
    const MsmJob job = jobs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x * per_wg >= job.n && blockIdx.x) return;   // (jobs of a launch differ in size: nothing of this one here)
    for (uint32_t t = tid; t < n_coarse; t += blockDim.x) h[t] = 0;
    __syncthreads();
    for (uint32_t e = 0; e < per_wg / 256; e++) {
        const uint32_t i = blockIdx.x * per_wg + e * 256 + tid;
        if (i >= job.n || msm_job_pos(job, sels, blockIdx.y, i) < 0) continue;
        msm_digits(job, i, c, rc, [&](uint32_t, uint32_t, uint32_t mag, bool) { atomicAdd(&h[(mag >> 1) >> fine_log], 1u); });
    }
    __syncthreads();
    uint32_t* bb = blockbase + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n_coarse;
    uint32_t* jc = coarse_cnt + (size_t)blockIdx.y * n_coarse;
    for (uint32_t t = tid; t < n_coarse; t += blockDim.x) bb[t] = h[t] ? atomicAdd(&jc[t], h[t]) : 0u;
}

// Exclusive scan over the nt threads of the workgroup of K values per thread (Hillis-Steele in K LDS arrays of nt words, ONE
// pair of barriers per step for all K): v[k] comes back as the sum of the v[k] of the threads below, and part[k][t] is left
// holding the inclusive sum of thread t - part[k][nt - 1] the total.
template <int K>
ZK_DI void block_scan_excl(uint32_t* const (&part)[K], uint32_t (&v)[K], uint32_t tid, uint32_t nt) {
#pragma unroll
    for (int k = 0; k < K; k++) part[k][tid] = v[k];
    __syncthreads();
    for (uint32_t d = 1; d < nt; d <<= 1) {
        uint32_t below[K];
#pragma unroll
        for (int k = 0; k < K; k++) below[k] = tid >= d ? part[k][tid - d] : 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; k++) part[k][tid] += below[k];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = tid ? part[k][tid - 1] : 0;
}

// exclusive scan of n values per job (n <= a few thousand), one workgroup per job; total[job] = sum
static __global__ void __launch_bounds__(1024)
k_msm_coarse_scan(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ total, uint32_t n) {
    ZK_SHARED uint32_t part[1024];
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t per = (n + nt - 1) / nt;
    const uint32_t* src = in + (size_t)blockIdx.x * n;
    uint32_t* dst = out + (size_t)blockIdx.x * n;
    uint32_t e0 = tid * per, e1 = e0 + per < n ? e0 + per : n;
    if (e0 > n) e0 = n;
    uint32_t sum[1] = {0};
    for (uint32_t e = e0; e < e1; e++) sum[0] += src[e];
    uint32_t* const lds[1] = {part};
    block_scan_excl(lds, sum, tid, nt);
    uint32_t run = sum[0];
    for (uint32_t e = e0; e < e1; e++) {
        const uint32_t k = src[e];
        dst[e] = run;
        run += k;
    }
    if (total && tid == nt - 1) total[blockIdx.x] = part[nt - 1];
}

// record = (bucket inside its coarse bin, pair);  pair = (table index << 1) | sign,
// table index = position * n_table + base
static __global__ void __launch_bounds__(256)
k_msm_coarse_scatter(const MsmJob* __restrict__ jobs, uint32_t c, uint32_t fine_log, uint32_t n_coarse,
                     const uint32_t* __restrict__ coarse_off, const uint32_t* __restrict__ blockbase, uint2* __restrict__ rec,
                     uint32_t per_wg, const MsmSelSet sels = MsmSelSet{}, const MsmRecode rc = MsmRecode{}) {
    ZK_SHARED uint32_t h[MSM_COARSE_MAX];
    const MsmJob job = jobs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x * per_wg >= job.n && blockIdx.x) return;
    const uint32_t* bb = blockbase + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n_coarse;
    const uint32_t* jo = coarse_off + (size_t)blockIdx.y * n_coarse;
    for (uint32_t t = tid; t < n_coarse; t += blockDim.x) h[t] = jo[t] + bb[t];
    __syncthreads();
    uint2* jrec = rec + job.pair_base;
    const uint32_t fmask = (1u << fine_log) - 1;
    for (uint32_t e = 0; e < per_wg / 256; e++) {
        const uint32_t i = blockIdx.x * per_wg + e * 256 + tid;
        if (i >= job.n) continue;
        const int32_t pos = msm_job_pos(job, sels, blockIdx.y, i);
        if (pos < 0) continue;
        const uint32_t tbase = job.table_base + (uint32_t)pos, tstride = job.n_table;
        msm_digits(job, i, c, rc, [&](uint32_t, uint32_t bit, uint32_t mag, bool negative) {
            const uint32_t b = mag >> 1;
            const uint32_t slot = atomicAdd(&h[b >> fine_log], 1u);
            jrec[slot] = make_uint2(b & fmask, ((tbase + bit * tstride) << 1) | (negative ? 1u : 0u));
        });
    }
}

// The layout of m buckets from their pair counts in the LDS histogram h[0 .. m): exclusive scans over the workgroup of the
// counts (pair slots) and of the task counts - a bucket with k points is cut into ceil(k / seg) tasks (see below) - thread t
// owning the buckets [t * per, ..).  Bucket b gets cnt[b], off[b] = `first` + its first pair slot, toff[b] = its first task;
// h[b] is left as the bucket's slot cursor, relative to the first pair of the m buckets.  The caller holds a barrier before the
// cursors are used.  Returns the task count up to and including the thread's buckets: in thread nt - 1, the total.
ZK_DI uint32_t msm_bucket_layout(uint32_t* h, uint32_t m, uint32_t first, uint32_t* cnt, uint32_t* off, uint32_t* toff, uint32_t seg,
                                 uint32_t* part, uint32_t* tpart, uint32_t tid, uint32_t nt) {
    const uint32_t per = (m + nt - 1) / nt;
    uint32_t b0 = tid * per, b1 = b0 + per < m ? b0 + per : m;
    if (b0 > m) b0 = m;
    uint32_t run[2] = {0, 0};   // pairs, tasks
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t k = h[b];
        run[0] += k;
        run[1] += (k + seg - 1) / seg;
    }
    uint32_t* const lds[2] = {part, tpart};
    block_scan_excl(lds, run, tid, nt);
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t k = h[b];
        cnt[b] = k;
        off[b] = first + run[0];
        toff[b] = run[1];
        h[b] = run[0];
        run[0] += k;
        run[1] += (k + seg - 1) / seg;
    }
    return tpart[tid];
}

// grid (coarse bins, jobs).  A bucket with k points is cut into ceil(k / seg) tasks (see below);
// toff is left relative to the bin's first task, bin_tasks[bin] = tasks of the bin.
static __global__ void __launch_bounds__(1024)
k_msm_fine_sort(const MsmJob* __restrict__ jobs, const uint2* __restrict__ rec, const uint32_t* __restrict__ coarse_cnt,
                const uint32_t* __restrict__ coarse_off, uint32_t fine, uint32_t nb, uint32_t* cnt, uint32_t* off, uint32_t* toff,
                uint32_t* bin_tasks, uint32_t* pairs, uint32_t seg) {
    ZK_SHARED uint32_t h[MSM_FINE_MAX];
    ZK_SHARED uint32_t part[1024];
    ZK_SHARED uint32_t tpart[1024];
    const uint32_t tid = threadIdx.x, nt = blockDim.x, bin = blockIdx.x, n_coarse = gridDim.x;
    const MsmJob job = jobs[blockIdx.y];
    const uint32_t n_rec = coarse_cnt[(size_t)blockIdx.y * n_coarse + bin];
    const uint32_t first = job.pair_base + coarse_off[(size_t)blockIdx.y * n_coarse + bin];
    for (uint32_t t = tid; t < fine; t += nt) h[t] = 0;
    __syncthreads();
    {
        // four records in flight per thread
        uint32_t e = tid;
        for (; e + 3 * nt < n_rec; e += 4 * nt) {
            const uint32_t k0 = rec[first + e].x, k1 = rec[first + e + nt].x, k2 = rec[first + e + 2 * nt].x,
                           k3 = rec[first + e + 3 * nt].x;
            atomicAdd(&h[k0], 1u);
            atomicAdd(&h[k1], 1u);
            atomicAdd(&h[k2], 1u);
            atomicAdd(&h[k3], 1u);
        }
        for (; e < n_rec; e += nt) atomicAdd(&h[rec[first + e].x], 1u);
    }
    __syncthreads();
    // (the slot cursors are relative to the bin's first pair, toff to the bin's first task)
    const size_t b0 = (size_t)blockIdx.y * nb + (size_t)bin * fine;
    const uint32_t tasks = msm_bucket_layout(h, fine, first, cnt + b0, off + b0, toff + b0, seg, part, tpart, tid, nt);
    if (tid == nt - 1) bin_tasks[(size_t)blockIdx.y * n_coarse + bin] = tasks;
    __syncthreads();
    uint32_t e = tid;
    for (; e + 3 * nt < n_rec; e += 4 * nt) {
        const uint2 r0 = rec[first + e], r1 = rec[first + e + nt], r2 = rec[first + e + 2 * nt], r3 = rec[first + e + 3 * nt];
        const uint32_t s0 = atomicAdd(&h[r0.x], 1u), s1 = atomicAdd(&h[r1.x], 1u), s2 = atomicAdd(&h[r2.x], 1u),
                       s3 = atomicAdd(&h[r3.x], 1u);
        pairs[first + s0] = r0.y;
        pairs[first + s1] = r1.y;
        pairs[first + s2] = r2.y;
        pairs[first + s3] = r3.y;
    }
    for (; e < n_rec; e += nt) {
        const uint2 r = rec[first + e];
        pairs[first + atomicAdd(&h[r.x], 1u)] = r.y;
    }
}

// toff[b] += first task of b's bin; grid (blocks over the buckets, jobs)
static __global__ void __launch_bounds__(256)
k_msm_task_offsets(uint32_t* toff, const uint32_t* __restrict__ bin_tbase, uint32_t nb, uint32_t fine_log, uint32_t n_coarse) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) toff[(size_t)blockIdx.y * nb + b] += bin_tbase[(size_t)blockIdx.y * n_coarse + (b >> fine_log)];
}

// Passes 1-3 fused for jobs whose bucket histogram fits LDS (every per-proof job): one workgroup
// per job counts the digits in an LDS histogram, scans it in place (writing cnt / off / toff for
// the later passes) and scatters the pairs with LDS tickets.  No global atomics at all; the
// two-level path above is for histograms that do not fit.
// (two workgroups of sixteen waves per CU: 64 VGPRs - the recoding over the multiples took 76 without the second bound, one
//  workgroup per CU, and every sort 2 ms longer)
static __global__ void __launch_bounds__(MSM_SORT_THREADS, 8)
k_msm_sort_lds(const MsmJob* __restrict__ jobs, uint32_t c, uint32_t* cnt, uint32_t* off, uint32_t* toff,
               uint32_t* ntasks, uint32_t* pairs, uint32_t seg, uint32_t dbg, const MsmSelSet sels = MsmSelSet{},
               const MsmRecode rc = MsmRecode{}) {
    ZK_DYN_SHARED(uint32_t, h);   // [nb] histogram, then running slot cursors
    ZK_SHARED uint32_t part[MSM_SORT_THREADS];
    ZK_SHARED uint32_t tpart[MSM_SORT_THREADS];
    const MsmJob job = jobs[blockIdx.x];
    const uint32_t nb = 1u << (c - 2), tid = threadIdx.x, nt = MSM_SORT_THREADS;
    for (uint32_t b = tid; b < nb; b += nt) h[b] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < job.n; i += nt) {
        if (msm_job_pos(job, sels, blockIdx.x, i) < 0) continue;
        msm_digits(job, i, c, rc, [&](uint32_t, uint32_t, uint32_t mag, bool) { atomicAdd(&h[mag >> 1], 1u); });
    }
    __syncthreads();
    // (the slot cursors are relative to the job's first pair)
    const size_t row = (size_t)blockIdx.x * nb;
    const uint32_t tasks = msm_bucket_layout(h, nb, job.pair_base, cnt + row, off + row, toff + row, seg, part, tpart, tid, nt);
    if (tid == nt - 1) ntasks[blockIdx.x] = tasks;
    __syncthreads();
    uint32_t* jpairs = pairs + job.pair_base;
    if (dbg & 2u) return;   // diagnostics (ZKAMD_DEBUG_SORT): the count pass and the scan alone
    for (uint32_t i = tid; i < job.n; i += nt) {
        const int32_t pos = msm_job_pos(job, sels, blockIdx.x, i);
        if (pos < 0) continue;
        const uint32_t tbase = job.table_base + (uint32_t)pos, tstride = job.n_table;
        msm_digits(job, i, c, rc, [&](uint32_t, uint32_t bit, uint32_t mag, bool negative) {
            uint32_t slot = atomicAdd(&h[mag >> 1], 1u);
            if ((dbg & 1u) && slot != 0xffffffffu) return;   // diagnostics: everything but the scattered store
            jpairs[slot] = ((tbase + bit * tstride) << 1) | (negative ? 1u : 0u);
        });
    }
}

// A bucket of k points becomes nt = ceil(k / seg) tasks of EQUAL length (n_long of len + 1 points,
// then n_short of len): the tasks of a launch run in rounds over the thread slots of the GPU, and a
// round lasts as long as its longest task - cutting 102 points into 64 + 38 instead of 51 + 51 left
// a third of the lanes idle on a single large job (VALU 64 % busy, 3.1 ms).
struct TaskCut {
    uint32_t n_long, n_short, len;
};
ZK_DI TaskCut task_cut(uint32_t k, uint32_t seg) {
    if (!k) return TaskCut{0, 0, 1};
    const uint32_t nt = (k + seg - 1) / seg;
    return TaskCut{k % nt, nt - k % nt, k / nt};
}

// Pass 4a: histogram of task lengths (1 .. seg) per job.  One thread per bucket.
static __global__ void __launch_bounds__(256)
k_msm_task_hist(const uint32_t* __restrict__ cnt, uint32_t* lenhist, uint32_t nb, uint32_t seg) {
    ZK_SHARED uint32_t h[MSM_SEG_MAX];
    const uint32_t tid = threadIdx.x, job = blockIdx.y;
    if (tid < seg) h[tid] = 0;
    __syncthreads();
    uint32_t b = blockIdx.x * blockDim.x + tid;
    if (b < nb) {
        const TaskCut tc = task_cut(cnt[(size_t)job * nb + b], seg);
        if (tc.n_long) atomicAdd(&h[tc.len], tc.n_long);
        if (tc.n_short) atomicAdd(&h[tc.len - 1], tc.n_short);
    }
    __syncthreads();
    if (tid < seg && h[tid]) atomicAdd(&lenhist[(size_t)job * seg + tid], h[tid]);
}

// Pass 4b: first slot of every (length, job) class in the launch-wide task order: longest tasks
// first, jobs in order inside a length class.  One workgroup.
static __global__ void __launch_bounds__(1024)
k_msm_task_base(const uint32_t* __restrict__ lenhist, uint32_t* base, uint32_t* total, uint32_t nj, uint32_t seg) {
    ZK_SHARED uint32_t part[1024];
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t E = nj * seg;
    const uint32_t per = (E + nt - 1) / nt;
    uint32_t e0 = tid * per, e1 = e0 + per < E ? e0 + per : E;
    if (e0 > E) e0 = E;
    // entry e = (seg - 1 - len_index) * nj + job
    uint32_t sum[1] = {0};
    for (uint32_t e = e0; e < e1; e++) sum[0] += lenhist[(size_t)(e % nj) * seg + (seg - 1 - e / nj)];
    uint32_t* const lds[1] = {part};
    block_scan_excl(lds, sum, tid, nt);
    uint32_t run = sum[0];
    for (uint32_t e = e0; e < e1; e++) {
        base[e] = run;
        run += lenhist[(size_t)(e % nj) * seg + (seg - 1 - e / nj)];
    }
    if (tid == nt - 1) total[0] = part[nt - 1];
}

// Pass 4c: write the task descriptors {first pair, index of the partial sum, length} in that
// order.  A workgroup reserves a range per length class with one global atomic, its threads
// take slots inside the range from LDS counters.
static __global__ void __launch_bounds__(256)
k_msm_task_place(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, const uint32_t* __restrict__ toff,
                 const uint32_t* __restrict__ task_base, const uint32_t* __restrict__ base, uint32_t* cursor,
                 uint4* sorted, uint32_t* n_heavy, uint32_t* heavy, uint32_t nb, uint32_t nj, uint32_t merge_inline,
                 uint32_t seg, uint32_t* n_light, uint32_t* light) {
    ZK_SHARED uint32_t h[MSM_SEG_MAX];
    ZK_SHARED uint32_t start[MSM_SEG_MAX];
    ZK_SHARED uint32_t lists[4];   // heavy / light buckets of this workgroup, then the two ranges it reserved
    const uint32_t tid = threadIdx.x, job = blockIdx.y;
    if (tid < seg) h[tid] = 0;
    if (tid < 4) lists[tid] = 0;
    __syncthreads();
    uint32_t b = blockIdx.x * blockDim.x + tid;
    TaskCut tc = {0, 0, 1};
    if (b < nb) {
        tc = task_cut(cnt[(size_t)job * nb + b], seg);
        if (tc.n_long) atomicAdd(&h[tc.len], tc.n_long);
        if (tc.n_short) atomicAdd(&h[tc.len - 1], tc.n_short);
    }
    __syncthreads();
    if (tid < seg) {
        uint32_t n = h[tid];
        start[tid] = base[(size_t)(seg - 1 - tid) * nj + job] + (n ? atomicAdd(&cursor[(size_t)job * seg + tid], n) : 0u);
        h[tid] = 0;
    }
    __syncthreads();
    // the heavy / light lists: slots are taken from LDS counters and ONE global atomic per workgroup and list reserves the
    // range (a variable-base multiexp has every bucket on the light list: 155 000 atomics on one address were 1.5 ms)
    {
        const uint32_t nt_b = tc.n_long + tc.n_short;
        const bool is_heavy = b < nb && nt_b > merge_inline, is_light = b < nb && !is_heavy && light && nt_b > 1;   // light: 2 .. merge_inline partials
        uint32_t slot = 0;
        if (is_heavy) slot = atomicAdd(&lists[0], 1u);
        if (is_light) slot = atomicAdd(&lists[1], 1u);
        __syncthreads();
        if (tid < 2 && lists[tid]) lists[2 + tid] = atomicAdd(tid ? n_light : n_heavy, lists[tid]);
        __syncthreads();
        if (is_heavy) heavy[lists[2] + slot] = job * nb + b;
        if (is_light) light[lists[3] + slot] = job * nb + b;
    }
    if (tc.n_long + tc.n_short) {
        const uint32_t o = off[(size_t)job * nb + b], ti = task_base[job] + toff[(size_t)job * nb + b];
        if (tc.n_long) {
            uint32_t at = start[tc.len] + atomicAdd(&h[tc.len], tc.n_long);
            for (uint32_t i = 0; i < tc.n_long; i++) sorted[at + i] = make_uint4(o + i * (tc.len + 1), ti + i, tc.len + 1, 0);
        }
        const uint32_t o2 = o + tc.n_long * (tc.len + 1), at = start[tc.len - 1] + atomicAdd(&h[tc.len - 1], tc.n_short);
        for (uint32_t i = 0; i < tc.n_short; i++) sorted[at + i] = make_uint4(o2 + i * tc.len, ti + tc.n_long + i, tc.len, 0);
    }
}

}  // namespace zkdev
