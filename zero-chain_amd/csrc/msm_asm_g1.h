// The wrappers of the generated G1 loops (overview: msm.h): the accumulation (madd_asm.h) and level 1 of the bucket reduction
// (red_asm.h).  msm_g1.cpp alone includes this header - and with it the ~29 000 generated lines - and launches its kernels.
#pragma once
#include "msm_accumulate.h"
#ifdef ZK_HAVE_MADD_ASM
#include "madd_asm.h"
#include "red_asm.h"

namespace zkdev {

// Pass 5, G1: the whole loop as ONE generated assembly body (madd_asm.h, tools/gen_madd_asm.py): every product is
// emitted in place over the registers its operands live in, the modulus stays in SGPRs, 160 VGPRs = three waves per
// SIMD (the compiled loop above: 198 VGPRs, two waves, ~390 operand moves per addition), and inside the loop the field
// is SIGNED and lazily reduced - a difference is one limb-wise subtraction, no multiple of p, no carry pass - with
// the accumulator's y held as sigma * Y, sigma = -1 after every second step (see the generator).  The loop computes
// the generic madd-2008-s formula only; a step that meets P == +-acc leaves ZZ == 0 (mod p), which every later step
// preserves, so ONE test per task after the loop queues the task for k_msm_accumulate_redo (the compiled loop with
// all special cases).  The first point of a task initialises the accumulator here, the assembly adds points
// 1 .. n - 1, and the four coordinates return to the unsigned weakly normalised form of dev_field.h below.
ZK_DI void g1asm_task(uint32_t t, const Affine<Fq28>* __restrict__ table, const uint32_t* __restrict__ pairs,
                       const uint4* __restrict__ sorted, XYZZ<Fq28>* __restrict__ tsums, uint32_t* __restrict__ n_redo,
                       uint32_t* __restrict__ redo) {
    static_assert(ZK_MADD_G1_VGPRS <= 168, "the loop must fit three waves per SIMD");
    static_assert(XYZZ<Fq28>::BX >= 9 && XYZZ<Fq28>::BY >= 5, "bounds of the values handed back by the loop");
    const uint4 d = sorted[t];
    const uint32_t n = d.z;
    XYZZ<Fq28> acc = XYZZ<Fq28>::inf();
    if (n) {
        const uint32_t* pp = pairs + d.x;
        const uint32_t pr = pp[0];
        const Affine<Fq28> p = table[pr >> 1];
        if (n == 1) {
            acc = XYZZ<Fq28>{p.x, (pr & 1u) ? neg_b<Fq28::MO>(p.y) : p.y, Fq28::one(), Fq28::one()};
        } else {
            u32x16 X = fq28_vec(p.x), Y = fq28_vec(p.y), ZZ = fq28_vec(Fq28::one()), ZZZ = ZZ;
            if (pr & 1u) {
#pragma unroll
                for (int i = 0; i < 14; i++) Y[i] = 0u - Y[i];   // W = -y as signed limbs (sigma = +1)
            }
            // the loop state rides in the pad registers of the operand blocks
            const uint64_t pa = (uint64_t)(uintptr_t)pp, ta = (uint64_t)(uintptr_t)table;
            X[14] = (uint32_t)pa;
            X[15] = (uint32_t)(pa >> 32);
            Y[14] = n;
            ZZ[14] = (uint32_t)ta;
            ZZ[15] = (uint32_t)(ta >> 32);
            asm volatile(ZK_MADD_G1_ASM
                         : "+{v[0:15]}"(X), "+{v[16:31]}"(Y), "+{v[32:47]}"(ZZ), "+{v[48:63]}"(ZZZ)
                         :
                         : ZK_MADD_G1_ASM_CLOBBERS);
            acc.x = fq28_from_signed<7, false>(X);                       // X in (-6 p, 2 p)      -> < 9 p
            acc.y = ((n - 1) & 1u) ? fq28_from_signed<3, true>(Y)        // W = -Y in (-0.07 p, 2 p) -> Y < 3.07 p
                                   : fq28_from_signed<2, false>(Y);      // W = +Y                -> Y < 4 p
            acc.zz = fq28_from_signed_product(ZZ);
            acc.zzz = fq28_from_signed_product(ZZZ);
            if (acc.zz.is_zero_norm()) redo[atomicAdd(n_redo, 1u)] = t;
        }
    }
    tsums[d.y] = acc;
}
static __global__ void __launch_bounds__(128, 3)
k_msm_accumulate_g1asm(const Affine<Fq28>* __restrict__ table, const uint32_t* __restrict__ pairs,
                       const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<Fq28>* __restrict__ tsums,
                       uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total[0]) g1asm_task(t, table, pairs, sorted, tsums, n_redo, redo);
}
// The same as a PERSISTENT launch (ZKAMD_G1_PERSIST = workgroups per CU): a fixed number of workgroups, every wave
// fetching blocks of 64 consecutive tasks from a counter.  With 4 workgroups per CU the launch holds two of the three
// wave slots its registers allow, so the short kernels of the other pipeline lane (NTT passes, sort, witness levels,
// reduction tails: up to 184 registers) find room on every SIMD while it runs instead of waiting for its workgroups
// to retire (r03final2 trace: a 3 ms pass of the other lane stretched to 114 ms beside a full-occupancy launch).
static __global__ void __launch_bounds__(128, 3)
k_msm_accumulate_g1asm_persistent(const Affine<Fq28>* __restrict__ table, const uint32_t* __restrict__ pairs,
                                  const uint4* __restrict__ sorted, const uint32_t* __restrict__ total,
                                  XYZZ<Fq28>* __restrict__ tsums, uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo,
                                  uint32_t* __restrict__ next) {
    const uint32_t ntask = total[0], lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(next, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= ntask) break;
        if (base + lane < ntask) g1asm_task(base + lane, table, pairs, sorted, tsums, n_redo, redo);
    }
}

// Pass 6, level 1, G1: the generated assembly loop of red_asm.h (tools/gen_red_asm.py).  One thread per node of L
// buckets walks them from the top down with BOTH accumulators in registers (run = the suffix sum R_k, acc = sum of R_k
// over k >= 1) and writes S = R_0 and A = acc: nothing but the bucket sums is read, no suffix array goes through HBM
// (k_msm_suffix_buckets + k_msm_segsum: 224 B read, 224 B written and 224 B read again per bucket), and the XYZZ full
// addition is ~6 100 in-place instructions against the compiled one's ~9 000 through the out-of-line product routines.
// Every bucket must hold ONE partial: the launch runs behind k_msm_merge_heavy with all multi-task buckets merged.
// The tail above it forms W = 2 A + S (coop_tail.cpp k_ct_upper, w_is_a).  Equal / opposite operands and buckets that are the point at
// infinity leave ZZ == 0 (mod p) in the result they entered; such a node is recomputed here by the compiled addition.
ZK_DI XYZZ<Fq28> red_asm_point(const u32x16& x, const u32x16& y, const u32x16& zz, const u32x16& zzz, bool is_inf, bool raw) {
    if (is_inf) return XYZZ<Fq28>::inf();
    if (raw) return XYZZ<Fq28>{fq28_unvec(x), fq28_unvec(y), fq28_unvec(zz), fq28_unvec(zzz)};   // copied as it was loaded
    return XYZZ<Fq28>{fq28_from_signed<7, false>(x),       // X in (-6 p, 2 p)                 -> < 9 p
                      fq28_from_signed<2, false>(y),       // Y: one reduction of two products, (-0.1 p, 1.1 p) -> < 4 p
                      fq28_from_signed_product(zz), fq28_from_signed_product(zzz)};
}
static __global__ void __launch_bounds__(64, 2)
k_msm_reduce1_g1asm(const XYZZ<Fq28>* __restrict__ tsums, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ toff,
                    const uint32_t* __restrict__ task_base, XYZZ<Fq28>* __restrict__ S, XYZZ<Fq28>* __restrict__ A, uint32_t nb,
                    uint32_t L, uint32_t* __restrict__ n_fallback) {
    static_assert(ZK_RED_G1_VGPRS <= 256, "the loop must fit two waves per SIMD");
    static_assert(sizeof(XYZZ<Fq28>) == 224, "the loop loads 224-byte partial sums");
    const uint32_t T = nb / L;
    const uint32_t bx = (blockIdx.x + blockIdx.y) % gridDim.x;   // XCD rotation, as in k_msm_suffix_buckets
    const uint32_t t = bx * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint32_t job = blockIdx.y;
    const size_t b0 = (size_t)job * nb + (size_t)t * L;
    const XYZZ<Fq28>* ts = tsums + task_base[job];
    u32x16 X = {}, Y = {}, ZZ = {}, ZZZ = {}, AX, AY, AZZ, AZZZ;
    const uint64_t pc = (uint64_t)(uintptr_t)(cnt + b0), pt = (uint64_t)(uintptr_t)(toff + b0), pp = (uint64_t)(uintptr_t)ts;
    X[14] = (uint32_t)pc;
    X[15] = (uint32_t)(pc >> 32);
    Y[14] = (uint32_t)pt;
    Y[15] = (uint32_t)(pt >> 32);
    ZZ[14] = (uint32_t)pp;
    ZZ[15] = (uint32_t)(pp >> 32);
    ZZZ[14] = L;
    asm volatile(ZK_RED_G1_ASM
                 : "+{v[0:15]}"(X), "+{v[16:31]}"(Y), "+{v[32:47]}"(ZZ), "+{v[48:63]}"(ZZZ), "={v[64:79]}"(AX), "={v[80:95]}"(AY),
                   "={v[96:111]}"(AZZ), "={v[112:127]}"(AZZZ)
                 :
                 : ZK_RED_G1_ASM_CLOBBERS);
    const uint32_t flags = ZZZ[15];
    XYZZ<Fq28> run = red_asm_point(X, Y, ZZ, ZZZ, (flags & ZK_RED_FLAG_RUN_INF) != 0, (flags & ZK_RED_FLAG_RUN_RAW) != 0);
    XYZZ<Fq28> acc = red_asm_point(AX, AY, AZZ, AZZZ, (flags & ZK_RED_FLAG_ACC_INF) != 0, (flags & ZK_RED_FLAG_ACC_RAW) != 0);
    if ((!(flags & ZK_RED_FLAG_RUN_INF) && run.zz.is_zero_norm()) || (!(flags & ZK_RED_FLAG_ACC_INF) && acc.zz.is_zero_norm())) {
        // a special case somewhere in the node (or a bucket whose points cancelled): the compiled addition knows them all
        atomicAdd(n_fallback, 1u);   // diagnostics (ZKAMD_DEBUG_REDO)
        run = XYZZ<Fq28>::inf();
        acc = XYZZ<Fq28>::inf();
        for (int k = (int)L - 1; k >= 0; k--) {
            if (cnt[b0 + k]) run = xadd(run, ts[toff[b0 + k]]);
            if (k >= 1) acc = xadd(acc, run);
        }
    }
    S[(size_t)job * T + t] = run;
    A[(size_t)job * T + t] = acc;
}
// The scratch-free second form of level 1 (see k_msm_accumulate_g2asm_sf): the lane index comes from the execution mask
// before and again after the loop, the clobber list names only what the loop touches, and a node with a special case is
// LISTED for k_msm_reduce1_redo instead of being recomputed here (a call of the out-of-line product routines gives a kernel
// a stack, i.e. scratch memory).
static __global__ void __launch_bounds__(64, 2)
k_msm_reduce1_g1asm_sf(const XYZZ<Fq28>* __restrict__ tsums, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ toff,
                       const uint32_t* __restrict__ task_base, XYZZ<Fq28>* __restrict__ S, XYZZ<Fq28>* __restrict__ A, uint32_t nb,
                       uint32_t L, uint32_t* __restrict__ n_fallback, uint32_t* __restrict__ fallback) {
    const uint32_t T = nb / L;
    const uint32_t bx = (blockIdx.x + blockIdx.y) % gridDim.x;   // XCD rotation, as in k_msm_suffix_buckets
    const uint32_t t = bx * 64u + lane_of_wave(0u);
    if (t >= T) return;
    const uint32_t job = blockIdx.y;
    size_t b0 = (size_t)job * nb + (size_t)t * L;
    const XYZZ<Fq28>* ts = tsums + task_base[job];
    u32x16 X = {}, Y = {}, ZZ = {}, ZZZ = {}, AX, AY, AZZ, AZZZ;
    const uint64_t pc = (uint64_t)(uintptr_t)(cnt + b0), pt = (uint64_t)(uintptr_t)(toff + b0), pp = (uint64_t)(uintptr_t)ts;
    X[14] = (uint32_t)pc;
    X[15] = (uint32_t)(pc >> 32);
    Y[14] = (uint32_t)pt;
    Y[15] = (uint32_t)(pt >> 32);
    ZZ[14] = (uint32_t)pp;
    ZZ[15] = (uint32_t)(pp >> 32);
    ZZZ[14] = L;
    asm volatile(ZK_RED_G1_ASM
                 : "+{v[0:15]}"(X), "+{v[16:31]}"(Y), "+{v[32:47]}"(ZZ), "+{v[48:63]}"(ZZZ), "={v[64:79]}"(AX), "={v[80:95]}"(AY),
                   "={v[96:111]}"(AZZ), "={v[112:127]}"(AZZZ)
                 :
                 : ZK_RED_G1_ASM_CLOBBERS_MIN);
    uint32_t opaque0 = 0;
    asm volatile("" : "+s"(opaque0));   // (so that the index below is computed again instead of being kept)
    const uint32_t t2 = bx * 64u + lane_of_wave(opaque0);
    const uint32_t flags = ZZZ[15];
    XYZZ<Fq28> run = red_asm_point(X, Y, ZZ, ZZZ, (flags & ZK_RED_FLAG_RUN_INF) != 0, (flags & ZK_RED_FLAG_RUN_RAW) != 0);
    XYZZ<Fq28> acc = red_asm_point(AX, AY, AZZ, AZZZ, (flags & ZK_RED_FLAG_ACC_INF) != 0, (flags & ZK_RED_FLAG_ACC_RAW) != 0);
    if ((!(flags & ZK_RED_FLAG_RUN_INF) && run.zz.is_zero_norm()) || (!(flags & ZK_RED_FLAG_ACC_INF) && acc.zz.is_zero_norm()))
        fallback[atomicAdd(n_fallback, 1u)] = job * T + t2;
    S[(size_t)job * T + t2] = run;
    A[(size_t)job * T + t2] = acc;
}
// the listed nodes again, by the compiled addition with all special cases (a few hundred of two million per launch set)
static __global__ void __launch_bounds__(64, MsmOcc<Fq28>::red)
k_msm_reduce1_redo(const XYZZ<Fq28>* __restrict__ tsums, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ toff,
                   const uint32_t* __restrict__ task_base, XYZZ<Fq28>* __restrict__ S, XYZZ<Fq28>* __restrict__ A, uint32_t nb,
                   uint32_t L, const uint32_t* __restrict__ n_fallback, const uint32_t* __restrict__ fallback) {
    const uint32_t T = nb / L, n = n_fallback[0];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t node = fallback[i], job = node / T, t = node % T;
        const size_t b0 = (size_t)job * nb + (size_t)t * L;
        const XYZZ<Fq28>* ts = tsums + task_base[job];
        XYZZ<Fq28> run = XYZZ<Fq28>::inf(), acc = XYZZ<Fq28>::inf();
        for (int k = (int)L - 1; k >= 0; k--) {
            if (cnt[b0 + k]) run = xadd(run, ts[toff[b0 + k]]);
            if (k >= 1) acc = xadd(acc, run);
        }
        S[node] = run;
        A[node] = acc;
    }
}

}  // namespace zkdev
#endif
