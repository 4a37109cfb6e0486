// ElGamal balance decryption on the GPU: the discrete logarithm x of v = x G over a bounded range, G the generator of the
// reference's keys and ciphertexts (FixedGenerators::NoteCommitmentRandomness).  Replaces the brute-force walk of
// Ciphertext::decrypt (core/proofs/src/no_std_aliases/elgamal.rs:85-108: up to 10^6 dependent additions on one core) by a
// baby-step giant-step search:
//   baby steps   { j G : 0 <= j < 2^b } in an open-addressed hash resident on the device (the handle of zk_elgamal_table)
//   giant steps  v - k M, M = 2^b G, k = 0 .. ceil(limit / 2^b) - 1; a hit j gives x = k 2^b + j, kept if x < limit
// The curve code is the witness kernels' (witness_gpu.h: Fr, fr_inv, to_ext, ext_add with d2).
//
// Kernels
//   k_dlog_multiples  out[j] = j (2^shift G) for j < lanes * steps: lane t starts at t (2^shift G) and walks by
//                     lanes (2^shift G); its points go back to affine form with ONE inversion (Montgomery's trick)
//   k_dlog_insert     one thread per baby step: its slot in the hash, claimed with a 64-bit compare-and-swap
//   k_dlog_probe      limit <= 2^b: one lookup of v per ciphertext, no arithmetic
//   k_dlog_search     limit > 2^b: one thread per (ciphertext, chunk of 2^w giant steps); the chunk's first point from the
//                     giant-step table (multiples of 2^w M, at most 2^16 of them), then SEARCH_BATCH steps per inversion
// Hash slot: fingerprint (32 bits of a hash of the affine coordinates) << 32 | (j + 1), 0 = empty; 2^(b+1) slots.  A
// fingerprint hit is confirmed against the table's full coordinates before it counts.
#pragma once
#include "witness_gpu.h"

namespace zkdlog {

using zkdev::Fr;
using zkdev::ld_fr;
using zkdev::st_fr;
using zkwitdev::EP;
using zkwitdev::JP;

constexpr uint32_t GIANT_MAX_LOG = 16;        // the giant-step table holds at most 2^16 points, whatever b and the limit
constexpr uint32_t BUILD_LANES_LOG = 14;      // lanes of k_dlog_multiples
constexpr uint32_t SEARCH_BATCH = 8;          // giant steps brought back to affine form per inversion
constexpr uint32_t SEARCH_LANES = 65536;      // resident threads of k_dlog_search (its scratch: 1 KB each)
constexpr unsigned long long NOT_FOUND = ~0ull;
// consts buffer: G (affine), 2 d, -M (affine), Montgomery form, 8 words each
enum { C_GX = 0, C_GY = 8, C_D2 = 16, C_NEG_MX = 24, C_MY = 32, C_WORDS = 40 };

// log2 of the giant steps one search thread walks from its table entry: the table then needs 2^(32 - b - w) <= 2^16
// entries for the largest limit, 2^32
inline uint32_t giant_stride_log(uint32_t baby_bits) {
    const int w = 32 - (int)baby_bits - (int)GIANT_MAX_LOG;
    return w > 3 ? (uint32_t)w : 3u;   // (at least one batch of SEARCH_BATCH steps)
}
static_assert(SEARCH_BATCH == 8, "a chunk of 2^3 giant steps is one batch");

struct Table {
    const uint32_t* xy;          // [2^b][2] Fr: j G, affine
    unsigned long long* slots;   // [2^(b+1)]
    uint32_t slot_mask, fp_mask;
};

ZK_DI uint64_t point_hash(const Fr& x, const Fr& y) {
    uint64_t h = (((uint64_t)x.l[1] << 32) | x.l[0]) ^ ((uint64_t)y.l[0] << 21) ^ y.l[1];
    h ^= h >> 33;   // murmur3's finaliser
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// j with j G == p, or -1
ZK_DI int32_t lookup(const Table& t, const JP& p) {
    const uint64_t h = point_hash(p.x, p.y);
    const uint32_t fp = (uint32_t)(h >> 32) & t.fp_mask;
    for (uint32_t s = (uint32_t)h & t.slot_mask;; s = (s + 1) & t.slot_mask) {   // (half the slots stay empty)
        const unsigned long long e = t.slots[s];
        if (!e) return -1;
        if ((uint32_t)(e >> 32) != fp) continue;
        const uint32_t j = (uint32_t)e - 1u;
        if (ld_fr(t.xy + (size_t)j * 16) == p.x && ld_fr(t.xy + (size_t)j * 16 + 8) == p.y) return (int32_t)j;
    }
}

static __global__ void __launch_bounds__(64)
k_dlog_multiples(uint32_t* xy, uint32_t* scratch, const uint32_t* consts, uint32_t shift, uint32_t lanes_log, uint32_t steps) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lanes = 1u << lanes_log;
    if (t >= lanes) return;
    const Fr d2 = ld_fr(consts + C_D2);
    EP base = zkwitdev::to_ext(JP{ld_fr(consts + C_GX), ld_fr(consts + C_GY)});
#pragma unroll 1
    for (uint32_t k = 0; k < shift; k++) base = zkwitdev::ext_add(base, base, d2);
    EP p = zkwitdev::to_ext(zkwitdev::neutral()), step = base;
#pragma unroll 1
    for (int bit = (int)lanes_log - 1; bit >= 0; bit--) {   // p = t base, step = lanes base
        p = zkwitdev::ext_add(p, p, d2);
        if ((t >> bit) & 1u) p = zkwitdev::ext_add(p, base, d2);
        step = zkwitdev::ext_add(step, step, d2);
    }
    // X, Y into the table, Z and the prefix product of the Zs into the scratch: entry j = t + i lanes (a wave writes one
    // contiguous run)
    Fr acc = Fr::one();
#pragma unroll 1
    for (uint32_t i = 0; i < steps; i++) {
        const size_t j = t + (size_t)i * lanes;
        st_fr(xy + j * 16, p.X);
        st_fr(xy + j * 16 + 8, p.Y);
        st_fr(scratch + j * 16, p.Z);
        st_fr(scratch + j * 16 + 8, acc);
        acc = mul(acc, p.Z);
        if (i + 1 < steps) p = zkwitdev::ext_add(p, step, d2);
    }
    Fr inv = zkwitdev::fr_inv(acc);
#pragma unroll 1
    for (uint32_t i = steps; i-- > 0;) {
        const size_t j = t + (size_t)i * lanes;
        const Fr zi = mul(inv, ld_fr(scratch + j * 16 + 8));
        inv = mul(inv, ld_fr(scratch + j * 16));
        st_fr(xy + j * 16, mul(ld_fr(xy + j * 16), zi));
        st_fr(xy + j * 16 + 8, mul(ld_fr(xy + j * 16 + 8), zi));
    }
}

static __global__ void __launch_bounds__(64)
k_dlog_insert(Table t, uint32_t count) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint64_t h = point_hash(ld_fr(t.xy + (size_t)j * 16), ld_fr(t.xy + (size_t)j * 16 + 8));
    const unsigned long long e = ((unsigned long long)((uint32_t)(h >> 32) & t.fp_mask) << 32) | (j + 1u);
    for (uint32_t s = (uint32_t)h & t.slot_mask;; s = (s + 1) & t.slot_mask)
        if (atomicCAS(&t.slots[s], 0ull, e) == 0ull) return;
}

struct Search {
    Table tab;
    const uint32_t* v;           // [n][2] Fr: left - dk right of every ciphertext, affine
    const uint32_t* giant;       // [chunks][2] Fr: e (2^w M), affine
    const uint32_t* consts;
    uint32_t* scratch;           // [SEARCH_BATCH][4][lanes] Fr: X, Y, Z, prefix product
    unsigned long long* res;     // [n], NOT_FOUND until a confirmed x < limit
    uint64_t limit, steps;       // steps = ceil(limit / 2^b)
    uint32_t n, baby_bits, w_log, chunks, lanes;
};

static __global__ void __launch_bounds__(64)
k_dlog_probe(Search s) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const int32_t j = lookup(s.tab, JP{ld_fr(s.v + (size_t)i * 16), ld_fr(s.v + (size_t)i * 16 + 8)});
    if (j >= 0 && (uint64_t)j < s.limit) s.res[i] = (unsigned long long)j;
}

static __global__ void __launch_bounds__(64)
k_dlog_search(Search s) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= s.lanes) return;
    const Fr d2 = ld_fr(s.consts + C_D2);
    const EP neg_m = zkwitdev::to_ext(JP{ld_fr(s.consts + C_NEG_MX), ld_fr(s.consts + C_MY)});
    auto slot = [&](uint32_t b, uint32_t c) { return s.scratch + ((size_t)(b * 4 + c) * s.lanes + lane) * 8; };
    const uint64_t items = (uint64_t)s.n * s.chunks;
#pragma unroll 1
    for (uint64_t u = lane; u < items; u += s.lanes) {
        const uint32_t i = (uint32_t)(u / s.chunks), e = (uint32_t)(u % s.chunks);
        const uint64_t k0 = (uint64_t)e << s.w_log;
        if (k0 >= s.steps) continue;
        const uint64_t k1 = k0 + (1ull << s.w_log) < s.steps ? k0 + (1ull << s.w_log) : s.steps;
        EP p = zkwitdev::to_ext(JP{ld_fr(s.v + (size_t)i * 16), ld_fr(s.v + (size_t)i * 16 + 8)});
        if (e) {   // v - e 2^w M
            const JP g{ld_fr(s.giant + (size_t)e * 16), ld_fr(s.giant + (size_t)e * 16 + 8)};
            p = zkwitdev::ext_add(p, zkwitdev::to_ext(JP{zkdev::neg(g.x), g.y}), d2);
        }
#pragma unroll 1
        for (uint64_t kb = k0; kb < k1; kb += SEARCH_BATCH) {
            const uint32_t nb = k1 - kb < SEARCH_BATCH ? (uint32_t)(k1 - kb) : SEARCH_BATCH;
            Fr acc = Fr::one();
#pragma unroll 1
            for (uint32_t b = 0; b < nb; b++) {   // p = v - (kb + b) M
                st_fr(slot(b, 0), p.X);
                st_fr(slot(b, 1), p.Y);
                st_fr(slot(b, 2), p.Z);
                st_fr(slot(b, 3), acc);
                acc = mul(acc, p.Z);
                p = zkwitdev::ext_add(p, neg_m, d2);
            }
            Fr inv = zkwitdev::fr_inv(acc);
#pragma unroll 1
            for (uint32_t b = nb; b-- > 0;) {
                const Fr zi = mul(inv, ld_fr(slot(b, 3)));
                inv = mul(inv, ld_fr(slot(b, 2)));
                const int32_t j = lookup(s.tab, JP{mul(ld_fr(slot(b, 0)), zi), mul(ld_fr(slot(b, 1)), zi)});
                if (j < 0) continue;
                const uint64_t x = ((kb + b) << s.baby_bits) + (uint64_t)j;
                if (x < s.limit) atomicMin(s.res + i, (unsigned long long)x);   // (one x at most: G has order ~2^252)
            }
        }
    }
}

}  // namespace zkdlog
