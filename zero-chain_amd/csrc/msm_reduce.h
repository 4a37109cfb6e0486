// Passes 5b, 5c and 6 of the multiexp on lanes (overview: msm.h): the task partials of a bucket merged into its first, then
// level 1 of the bucket reduction.  (On rows of 16 lanes: coop_tail.cpp; level 1 of G1 in assembly: msm_asm_g1.h.)
#pragma once
#include "dev_curve.h"
#include "msm_types.h"

namespace zkdev {

// Pass 5c: one thread sums the nt_b = 2 .. merge_inline partials of bucket gb into its first partial, so that the level-1
// threads of the reduction below, each a serial chain over L buckets, add one point per bucket.  With one large job
// the recoding's top digit alone gives ~2^(c-6) buckets twice the average load, i.e. a run of
// neighbouring buckets with 4 partials each.  Few jobs: the trailing workgroups of k_msm_merge_heavy, every bucket's
// thread looking whether it has something to merge; many jobs: k_msm_merge_light over the listed buckets.
template <class F>
ZK_DI void msm_merge_bucket(uint32_t gb, uint32_t nt_b, const uint32_t* __restrict__ toff, const uint32_t* __restrict__ task_base,
                            XYZZ<F>* tsums, uint32_t nb) {
    XYZZ<F>* ts = tsums + task_base[gb / nb] + toff[gb];
    XYZZ<F> acc = ts[0];
    for (uint32_t u = 1; u < nt_b; u++) acc = xadd(acc, ts[u]);
    ts[0] = acc;
}

// Pass 5b: buckets cut into many tasks.  Scalars are not uniform where it matters: the LAST digit
// of the recoding sits in whatever is left of the 254 bits above the previous digit, so a few small
// magnitudes collect a large share of all top digits (and boolean witnesses pile up on magnitude 1).
// Such a bucket yields hundreds of task partials; summing them inside the (one thread per 16
// buckets) reduction would leave the whole GPU waiting for one thread.  One workgroup per heavy
// bucket sums its partials with a strided pass and an LDS tree, and leaves the result in the
// bucket's first partial.
template <class F>
static __global__ void __launch_bounds__(MSM_MERGE_THREADS)
k_msm_merge_heavy(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ n_heavy, const uint32_t* __restrict__ cnt,
                  const uint32_t* __restrict__ toff, const uint32_t* __restrict__ task_base, XYZZ<F>* tsums, uint32_t nb,
                  uint32_t seg, uint32_t heavy_blocks, uint32_t light_buckets, uint32_t merge_inline, uint32_t min_tasks = 0) {
    ZK_SHARED XYZZ<F> sm[MSM_MERGE_THREADS];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x >= heavy_blocks) {
        // pass 5c inside the same launch (few jobs): the workgroups behind the first heavy_blocks take
        // one bucket per thread and sum its 2 .. merge_inline partials, beside - not after - the
        // heavy buckets' trees
        const uint32_t gb = (blockIdx.x - heavy_blocks) * MSM_MERGE_THREADS + tid;
        if (gb >= light_buckets) return;
        const uint32_t nt_b = (cnt[gb] + seg - 1) / seg;
        if (nt_b < 2 || nt_b > merge_inline) return;
        msm_merge_bucket(gb, nt_b, toff, task_base, tsums, nb);
        return;
    }
    // a fixed grid walks the list (launching one workgroup per POSSIBLE heavy bucket costs more than the work)
    for (uint32_t hb = blockIdx.x; hb < n_heavy[0]; hb += heavy_blocks) {
        const uint32_t gb = heavy[hb];
        const uint32_t nt = (cnt[gb] + seg - 1) / seg;
        if (nt <= min_tasks) continue;   // (k_msm_merge_medium's; uniform over the workgroup)
        XYZZ<F>* ts = tsums + task_base[gb / nb] + toff[gb];
        XYZZ<F> acc = XYZZ<F>::inf();
        for (uint32_t u = tid; u < nt; u += MSM_MERGE_THREADS) acc = xadd(acc, ts[u]);
        sm[tid] = acc;
        __syncthreads();
        for (uint32_t st = MSM_MERGE_THREADS / 2; st >= 1; st >>= 1) {
            if (tid < st) sm[tid] = xadd(sm[tid], sm[tid + st]);
            __syncthreads();
        }
        if (tid == 0) ts[0] = sm[0];
        __syncthreads();
    }
}

// Pass 5c, few-jobs sets whose heavy list is LONG (a variable-base multiexp with ~as many points per bucket as a task
// holds times merge_inline: half of the 24 k buckets of the 2^17-point G2 multiexp are "heavy" with 9 - 16 partials): a
// workgroup per bucket walks such a list for a millisecond - eight levels of a 256-wide tree for a dozen partials - so the
// listed buckets with at most max_tasks partials take EIGHT lanes each here (one or two partials per lane, three levels), eight
// buckets per workgroup and step; the few with more (the top digit position) keep the workgroup form / a workgroup of rows.
template <class F>
static __global__ void __launch_bounds__(64, MsmOcc<F>::red)
k_msm_merge_medium(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ n_heavy, const uint32_t* __restrict__ cnt,
                   const uint32_t* __restrict__ toff, const uint32_t* __restrict__ task_base, XYZZ<F>* tsums, uint32_t nb, uint32_t seg,
                   uint32_t max_tasks) {
    ZK_SHARED XYZZ<F> sm[64];
    const uint32_t tid = threadIdx.x, g = tid >> 3, r = tid & 7u, nh = n_heavy[0];
    for (uint32_t base = blockIdx.x * 8; base < nh; base += gridDim.x * 8) {
        const uint32_t hb = base + g;
        uint32_t nt = 0;
        XYZZ<F>* ts = nullptr;
        if (hb < nh) {
            const uint32_t gb = heavy[hb];
            nt = (cnt[gb] + seg - 1) / seg;
            if (nt > max_tasks) nt = 0;
            ts = tsums + task_base[gb / nb] + toff[gb];
        }
        XYZZ<F> acc = XYZZ<F>::inf();
        for (uint32_t u = r; u < nt; u += 8) acc = xadd(acc, ts[u]);
        sm[tid] = acc;
        __syncthreads();
        for (uint32_t st = 4; st >= 1; st >>= 1) {
            if (r < st && nt) sm[tid] = xadd(sm[tid], sm[tid + st]);
            __syncthreads();
        }
        if (r == 0 && nt) ts[0] = sm[tid];
        __syncthreads();
    }
}

// Pass 5c for the many-jobs launches: the buckets with 2 .. merge_inline partials (the small magnitudes that collect the
// top digits of the recoding: ~30 of a job's 8 192 buckets, ~60 000 per launch set) are LISTED by k_msm_task_place and
// merged here, one thread per listed bucket, every lane busy.  Left to the level-1 threads of the reduction they cost a
// serial chain of additions in one lane of a wave while its 63 neighbours wait (k_msm_suffix_buckets: 10.9 ms per launch
// set, the same again when every bucket's thread only looked whether it had something to merge: profiles/r04d).
template <class F>
static __global__ void __launch_bounds__(64, MsmOcc<F>::red)
k_msm_merge_light(const uint32_t* __restrict__ light, const uint32_t* __restrict__ n_light, const uint32_t* __restrict__ cnt,
                  const uint32_t* __restrict__ toff, const uint32_t* __restrict__ task_base, XYZZ<F>* tsums, uint32_t nb, uint32_t seg) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_light[0]; i += gridDim.x * blockDim.x) {
        const uint32_t gb = light[i];
        msm_merge_bucket(gb, (cnt[gb] + seg - 1) / seg, toff, task_base, tsums, nb);
    }
}

// Pass 6: bucket reduction  sum_j (2j + 1) * B_j  (bucket j holds the odd magnitude 2j + 1) by
// running sums.  A node covering L buckets carries
//     W = sum_b (2 (b - first) + 1) * B_b      (weights relative to the node's first bucket)
//     S = sum_b B_b
// With R_k = sum_{k' >= k} B_k' the suffix sums inside a node:
//     level 1:    S = R_0,  W = 2 * sum_{k >= 1} R_k + R_0                       (2 additions / bucket)
//     the tail:   sum_t W_t + 2L * sum_t t * S_t over the T nodes of a job, on rows of 16 lanes (coop_tail.cpp)
// No scalar multiplication anywhere (2L is a power of two: doublings), and every kernel below
// keeps exactly ONE point accumulator in registers: an extended-Jacobian addition with a second
// live accumulator does not fit 168 VGPRs next to the product routine's 40, and scratch spills
// inside these loops cost more than the arithmetic (measured: 5x on the batched prover, >100x on
// a single large job whose few waves cannot hide the spill latency).
//
// k_msm_suffix_buckets: R over the buckets (task partials merged on the fly), in bucket order.
template <class F>
static __global__ void __launch_bounds__(64, MsmOcc<F>::red)
k_msm_suffix_buckets(const XYZZ<F>* __restrict__ tsums, const uint32_t* __restrict__ cnt,
                     const uint32_t* __restrict__ toff, const uint32_t* __restrict__ task_base,
                     XYZZ<F>* __restrict__ R, uint32_t nb, uint32_t L, uint32_t merge_inline, uint32_t seg) {
    const uint32_t T = nb / L;
    // Workgroup (x, y) runs on XCD (y * gridDim.x + x) mod 8: with 8 workgroups per job the plain
    // mapping hands XCD 0 the lowest buckets of EVERY job - the ones with several task partials
    // (small top digits of the recoding) - and the launch waits for that XCD with the other SEs half
    // idle (SQ_BUSY_CYCLES / duration = 50 %).  Rotating the node range by the job index spreads them.
    const uint32_t bx = (blockIdx.x + blockIdx.y) % gridDim.x;
    uint32_t t = bx * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint32_t job = blockIdx.y;
    const size_t b0 = (size_t)job * nb + (size_t)t * L;
    const XYZZ<F>* ts = tsums + task_base[job];
    XYZZ<F> run = XYZZ<F>::inf();
    for (int k = (int)L - 1; k >= 0; k--) {
        uint32_t n = cnt[b0 + k];
        if (n) {
            uint32_t o = toff[b0 + k], nt_b = (n + seg - 1) / seg;
            if (nt_b > merge_inline) nt_b = 1;   // already summed into the first partial (k_msm_merge_heavy)
            for (uint32_t u = 0; u < nt_b; u++) run = xadd(run, ts[o + u]);
        }
        R[b0 + k] = run;
    }
}

// k_msm_segsum: per segment s of `seg` elements
//     acc = (init ? init[s] : 0) + sum_{first <= k < seg} in[s * seg + k]
//     out[s] = 2^dbl * acc + (plus_first ? in[s * seg] : 0)
template <class F>
static __global__ void __launch_bounds__(64, MsmOcc<F>::red)
k_msm_segsum(const XYZZ<F>* __restrict__ in, const XYZZ<F>* __restrict__ init, XYZZ<F>* __restrict__ out, uint32_t n,
             uint32_t seg, uint32_t first, uint32_t dbl, uint32_t plus_first) {
    const uint32_t ns = (n + seg - 1) / seg;
    uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= ns) return;
    const XYZZ<F>* p = in + (size_t)blockIdx.y * n;
    const uint32_t c0 = u * seg, c1 = c0 + seg < n ? c0 + seg : n;
    XYZZ<F> acc = init ? init[(size_t)blockIdx.y * ns + u] : XYZZ<F>::inf();
    for (uint32_t k = c0 + first; k < c1; k++) acc = xadd(acc, p[k]);
    for (uint32_t i = 0; i < dbl; i++) acc = xdbl(acc);
    if (plus_first) acc = xadd(acc, p[c0]);
    out[(size_t)blockIdx.y * ns + u] = acc;
}

}  // namespace zkdev
