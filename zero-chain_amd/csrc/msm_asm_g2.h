// The wrappers of the generated G2 loop (overview: msm.h; madd_asm.h ZK_MADD_G2_ASM) in its two forms.  msm_g2.cpp alone
// includes this header and launches its kernels.
#pragma once
#include "msm_accumulate.h"
#ifdef ZK_HAVE_MADD_ASM
#include "madd_asm.h"

namespace zkdev {

// Pass 5, G2: the same loop over Fq2 (madd_asm.h ZK_MADD_G2_ASM).  256 VGPRs = two waves per SIMD (the compiled
// kernel above: 468 registers, one wave): X and ZZ in registers, W = sigma Y and ZZZ parked in LDS (224 bytes per lane,
// [element quad][thread] x 16 bytes so that a wave's ds_read_b128 sweeps every bank once).
ZK_DI void g2asm_task(uint32_t t, uint4 (*park)[128], const Affine<Fq2x>* __restrict__ table, const uint32_t* __restrict__ pairs,
                       const uint4* __restrict__ sorted, XYZZ<Fq2x>* __restrict__ tsums, uint32_t* __restrict__ n_redo,
                       uint32_t* __restrict__ redo) {
    static_assert(ZK_MADD_G2_VGPRS <= 256, "the loop must fit two waves per SIMD");
    static_assert(ZK_MADD_G2_LDS_QUAD_STRIDE == 128 * 16, "parking area laid out for 128-thread workgroups");
    const uint4 d = sorted[t];
    const uint32_t n = d.z;
    XYZZ<Fq2x> acc = XYZZ<Fq2x>::inf();
    if (n) {
        const uint32_t* pp = pairs + d.x;
        const uint32_t pr = pp[0];
        const Affine<Fq2x> p = table[pr >> 1];
        if (n == 1) {
            acc = XYZZ<Fq2x>{p.x, (pr & 1u) ? neg_b<Fq2x::MO>(p.y) : p.y, Fq2x::one(), Fq2x::one()};
        } else {
            const uint32_t tid = threadIdx.x;
            auto put = [&](int slot, const Fq28& a, bool negate) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) w[j] = 4 * q + j < 14 ? (negate ? 0u - a.l[4 * q + j] : a.l[4 * q + j]) : 0u;
                    park[slot * 4 + q][tid] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            };
            auto get = [&](int slot) {
                u32x16 v;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint4 w = park[slot * 4 + q][tid];
                    v[4 * q] = w.x;
                    v[4 * q + 1] = w.y;
                    v[4 * q + 2] = w.z;
                    v[4 * q + 3] = w.w;
                }
                return v;
            };
            const Fq28 one = Fq28::one(), zero = Fq28::zero();
            put(ZK_MADD_G2_LDS_W, p.y.c0, (pr & 1u) != 0);        // W = +-y as signed limbs (sigma = +1)
            put(ZK_MADD_G2_LDS_W + 1, p.y.c1, (pr & 1u) != 0);
            put(ZK_MADD_G2_LDS_ZZZ, one, false);
            put(ZK_MADD_G2_LDS_ZZZ + 1, zero, false);
            u32x16 X0 = fq28_vec(p.x.c0), X1 = fq28_vec(p.x.c1), ZZ0 = fq28_vec(one), ZZ1 = fq28_vec(zero);
            const uint64_t pa = (uint64_t)(uintptr_t)pp, ta = (uint64_t)(uintptr_t)table;
            X0[14] = (uint32_t)pa;
            X0[15] = (uint32_t)(pa >> 32);
            X1[14] = n;
            ZZ0[14] = (uint32_t)ta;
            ZZ0[15] = (uint32_t)(ta >> 32);
            ZZ1[14] = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&park[0][tid];
            asm volatile(ZK_MADD_G2_ASM
                         : "+{v[0:15]}"(X0), "+{v[16:31]}"(X1), "+{v[32:47]}"(ZZ0), "+{v[48:63]}"(ZZ1)
                         :
                         : ZK_MADD_G2_ASM_CLOBBERS);
            const bool flip = ((n - 1) & 1u) != 0;
            // X is carry-normalised inside the loop, value in (-6 p, 2 p)
            acc.x = Fq2x{fq28_from_signed<7, false>(X0), fq28_from_signed<7, false>(X1)};
            const u32x16 w0 = get(ZK_MADD_G2_LDS_W), w1 = get(ZK_MADD_G2_LDS_W + 1);
            acc.y = flip ? Fq2x{fq28_from_signed<3, true>(w0), fq28_from_signed<3, true>(w1)}
                         : Fq2x{fq28_from_signed<2, false>(w0), fq28_from_signed<2, false>(w1)};
            acc.zz = Fq2x{fq28_from_signed_product(ZZ0), fq28_from_signed_product(ZZ1)};
            acc.zzz = Fq2x{fq28_from_signed_product(get(ZK_MADD_G2_LDS_ZZZ)), fq28_from_signed_product(get(ZK_MADD_G2_LDS_ZZZ + 1))};
            if (acc.zz.is_zero_norm()) redo[atomicAdd(n_redo, 1u)] = t;
        }
    }
    tsums[d.y] = acc;
}
static __global__ void __launch_bounds__(128, 2)
k_msm_accumulate_g2asm(const Affine<Fq2x>* __restrict__ table, const uint32_t* __restrict__ pairs,
                       const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<Fq2x>* __restrict__ tsums,
                       uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo) {
    ZK_SHARED uint4 park[16][128];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total[0]) g2asm_task(t, park, table, pairs, sorted, tsums, n_redo, redo);
}
// persistent form (see k_msm_accumulate_g1asm_persistent): a lane's LDS slots are its own, no barrier between tasks
static __global__ void __launch_bounds__(128, 2)
k_msm_accumulate_g2asm_persistent(const Affine<Fq2x>* __restrict__ table, const uint32_t* __restrict__ pairs,
                                  const uint4* __restrict__ sorted, const uint32_t* __restrict__ total,
                                  XYZZ<Fq2x>* __restrict__ tsums, uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo,
                                  uint32_t* __restrict__ next) {
    ZK_SHARED uint4 park[16][128];
    const uint32_t ntask = total[0], lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(next, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= ntask) break;
        if (base + lane < ntask) g2asm_task(base + lane, park, table, pairs, sorted, tsums, n_redo, redo);
    }
}
// ---- the SCRATCH-FREE second form of the G2 kernels (round 5; round 4's tools/experiments patch, now selected per device).
// A loop that owns all 256 VGPRs forces whatever the compiler keeps across it into scratch memory (the kernels above: 84 /
// 144 B per lane), and a dispatch that uses scratch runs under the runtime's scratch-wave limit: one box in seventeen ran
// exactly those kernels at a THIRD of their speed (profiles/r04k_*_slow_box.*).  Here nothing per-lane is live across the
// loop: its clobber list names only the registers it touches (ZK_MADD_G2_ASM_CLOBBERS_MIN), the task's (index, partial-sum
// slot, length) wait in LDS (`keep`), the thread index is formed again from the execution mask (`wbase` = first thread of the
// wave, uniform), and the constants of the conversion back are tied to a zero taken after the loop: 0 bytes of scratch.
// On a healthy box this form measured the same alone and 1.7 % slower in the overlapped step, so it is NOT the default:
// zkamd.cpp times both forms on the device when a key is loaded and takes this one only where the first is clearly slower.
ZK_DI void g2asm_task_sf(uint32_t t, uint32_t tid, uint32_t wbase, uint32_t z0, uint4 (*park)[128], uint4* keep, const Affine<Fq2x>* __restrict__ table,
                          const uint32_t* __restrict__ pairs, const uint4* __restrict__ sorted, XYZZ<Fq2x>* __restrict__ tsums,
                          uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo) {
    const uint4 d = sorted[t];
    const uint32_t n = d.z;
    if (n == 0) {
        tsums[d.y] = XYZZ<Fq2x>::inf();
        return;
    }
    const uint32_t* pp = pairs + d.x;
    const uint32_t pr = pp[0];
    const Affine<Fq2x> p = table[pr >> 1];
    if (n == 1) {
        tsums[d.y] = XYZZ<Fq2x>{p.x, (pr & 1u) ? neg_b<Fq2x::MO>(p.y) : p.y, Fq2x::one(), Fq2x::one()};
        return;
    }
    auto put = [&](int slot, const Fq28& a, bool negate) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = 4 * q + j < 14 ? (negate ? 0u - a.l[4 * q + j] : a.l[4 * q + j]) : 0u;
            park[slot * 4 + q][tid] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    // (constants of THIS round, tied to its opaque zero z0: as loop invariants they would be carried across the loop as
    //  whole 16-register vectors, in scratch)
    Fq28 one = Fq28::one(), zero;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        one.l[i] += z0;
        zero.l[i] = z0;
    }
    put(ZK_MADD_G2_LDS_W, p.y.c0, (pr & 1u) != 0);        // W = +-y as signed limbs (sigma = +1)
    put(ZK_MADD_G2_LDS_W + 1, p.y.c1, (pr & 1u) != 0);
    put(ZK_MADD_G2_LDS_ZZZ, one, false);
    put(ZK_MADD_G2_LDS_ZZZ + 1, zero, false);
    keep[tid] = make_uint4(t, d.y, n, n);   // (no constant in it: the compiler would carry the vector for its zero)
    u32x16 X0 = fq28_vec(p.x.c0), X1 = fq28_vec(p.x.c1), ZZ0 = fq28_vec(one), ZZ1 = fq28_vec(zero);
    const uint64_t pa = (uint64_t)(uintptr_t)pp, ta = (uint64_t)(uintptr_t)table;
    X0[14] = (uint32_t)pa;
    X0[15] = (uint32_t)(pa >> 32);
    X1[14] = n;
    X1[15] = z0;
    ZZ0[14] = (uint32_t)ta;
    ZZ0[15] = (uint32_t)(ta >> 32);
    ZZ1[14] = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&park[0][tid];
    ZZ1[15] = z0;
    asm volatile(ZK_MADD_G2_ASM
                 : "+{v[0:15]}"(X0), "+{v[16:31]}"(X1), "+{v[32:47]}"(ZZ0), "+{v[48:63]}"(ZZ1)
                 :
                 : ZK_MADD_G2_ASM_CLOBBERS_MIN);
    uint32_t z = 0;
    asm volatile("" : "+s"(z));
    const uint32_t tid2 = wbase + lane_of_wave(z);
    const uint4 kp = keep[tid2];   // (t, slot of the partial sum, n)
    auto get = [&](int slot) {
        u32x16 v;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 w = park[slot * 4 + q][tid2];
            v[4 * q] = w.x;
            v[4 * q + 1] = w.y;
            v[4 * q + 2] = w.z;
            v[4 * q + 3] = w.w;
        }
        return v;
    };
    const bool flip = ((kp.z - 1) & 1u) != 0;
    XYZZ<Fq2x> acc;
    acc.x = Fq2x{fq28_from_signed<7, false>(X0, z), fq28_from_signed<7, false>(X1, z)};
    const u32x16 w0 = get(ZK_MADD_G2_LDS_W), w1 = get(ZK_MADD_G2_LDS_W + 1);
    acc.y = flip ? Fq2x{fq28_from_signed<3, true>(w0, z), fq28_from_signed<3, true>(w1, z)}
                 : Fq2x{fq28_from_signed<2, false>(w0, z), fq28_from_signed<2, false>(w1, z)};
    acc.zz = Fq2x{fq28_from_signed_product(ZZ0, z), fq28_from_signed_product(ZZ1, z)};
    acc.zzz = Fq2x{fq28_from_signed_product(get(ZK_MADD_G2_LDS_ZZZ), z), fq28_from_signed_product(get(ZK_MADD_G2_LDS_ZZZ + 1), z)};
    // (indices widened with the opaque zero: a plain zero-extension takes its zero from a register set before the loop)
    const uint64_t zhi = (uint64_t)z << 32;
    if (acc.zz.is_zero_norm()) redo[atomicAdd(n_redo + z, 1u) | zhi] = kp.x;
    tsums[kp.y | zhi] = acc;
}
static __global__ void __launch_bounds__(128, 2)
k_msm_accumulate_g2asm_sf(const Affine<Fq2x>* __restrict__ table, const uint32_t* __restrict__ pairs,
                          const uint4* __restrict__ sorted, const uint32_t* __restrict__ total, XYZZ<Fq2x>* __restrict__ tsums,
                          uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo) {
    ZK_SHARED uint4 park[16][128];
    ZK_SHARED uint4 keep[128];
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u, tid = wbase + lane_of_wave(0u);
    const uint32_t t = blockIdx.x * blockDim.x + tid;
    uint32_t z = 0;
    asm volatile("" : "+s"(z));
    if (t < total[0]) g2asm_task_sf(t, tid, wbase, z, park, keep, table, pairs, sorted, tsums, n_redo, redo);
}
static __global__ void __launch_bounds__(128, 2)
k_msm_accumulate_g2asm_persistent_sf(const Affine<Fq2x>* __restrict__ table, const uint32_t* __restrict__ pairs,
                                     const uint4* __restrict__ sorted, const uint32_t* __restrict__ total,
                                     XYZZ<Fq2x>* __restrict__ tsums, uint32_t* __restrict__ n_redo, uint32_t* __restrict__ redo,
                                     uint32_t* __restrict__ next) {
    ZK_SHARED uint4 park[16][128];
    ZK_SHARED uint4 keep[128];
    const uint32_t ntask = total[0], wbase = __builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u;
    for (;;) {
        uint32_t z = 0;
        asm volatile("" : "+s"(z));                 // (the lane index is formed again in every round: see g2asm_task_sf)
        const uint32_t lane = lane_of_wave(z);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(next, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= ntask) break;
        if (base + lane < ntask) g2asm_task_sf(base + lane, wbase + lane, wbase, z, park, keep, table, pairs, sorted, tsums, n_redo, redo);
    }
}

// the tasks of the load-time comparison of the two forms (msm_g2.cpp calibrate_g2_accumulate; see msm_accumulate.h)
static __global__ void __launch_bounds__(256)
k_calib_tasks(uint32_t* pairs, uint4* sorted, uint32_t* total, uint32_t ntasks, uint32_t len, uint32_t n_table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) total[0] = ntasks;
    if (i < ntasks) sorted[i] = make_uint4(i * len, i, len, 0);
    if (i < ntasks * len) pairs[i] = ((calib_hash(i) % n_table) << 1) | (calib_hash(~i) & 1u);
}

}  // namespace zkdev
#endif
