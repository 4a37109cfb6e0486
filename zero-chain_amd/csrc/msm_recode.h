// The three recodings of a scalar into bucket digits (overview: msm.h): width-c NAF over the doubling table, the same over a
// table with odd multiples, and the regular recoding of the variable-base mode.  Device functions only: the sort kernels
// (msm_sort.h) and the hooks of the table multiples (msm_hooks.h) call msm_digits.
#pragma once
#include "msm_types.h"

namespace zkdev {

struct MsmConsts {
    static constexpr uint32_t R[8] = ZK_FR_P_32;
};

// The words a scalar is recoded from: s itself, or r - s with every sign flipped (`neg`) for s above (r - 1) / 2
// (s * P == (r - s) * (-P)), so the recoded value is < 2^254 and the last digit sits at a position <= 254.  False: the
// scalar has no digits.
ZK_DI bool msm_wnaf_words(const uint32_t* __restrict__ sp, uint32_t (&s)[8], bool& neg) {
    const uint4* q = reinterpret_cast<const uint4*>(sp);
    uint4 lo = q[0], hi = q[1];
    s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w;
    s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
    // t = r - s ; neg = (s > (r-1)/2)  <=>  (r - s) < s  <=>  t < s   (s < r assumed)
    uint32_t t[8], bo = 0, co;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        t[i] = __builtin_subc(MsmConsts::R[i], s[i], bo, &co);
        bo = co;
    }
    uint32_t lt = 0, decided = 0;   // compare t < s from the top word down
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        uint32_t l = (t[i] < s[i]) & ~decided, g = (t[i] > s[i]) & ~decided;
        lt |= l;
        decided |= l | g;
    }
    uint32_t zero_or = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) zero_or |= s[i];
    // s = 0 has no digits; neither has a NON-CANONICAL scalar (s >= r: r - s borrowed, or is zero).  The caller's canonical
    // test (k_fr_first_noncanonical, k_build_scalars) runs beside these launches and fails the call at its end; until then
    // the recoding must be total: a value >= 2^255 would put a digit at a position past the table's last slice.
    uint32_t t_or = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) t_or |= t[i];
    if (!zero_or || bo || !t_or) return false;
    neg = lt != 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = neg ? t[i] : s[i];
    return true;
}

// Width-c NAF of one scalar.  f(slot, position, odd magnitude in [1, 2^(c-1)), negative) is
// called for every non-zero digit, slot = 0, 1, 2 ... in order of increasing position.
// The sign normalisation is msm_wnaf_words'.  The words are consumed through a 64-bit shift buffer, so no dynamically
// indexed register array is needed.
template <class Fn>
ZK_DI void msm_wnaf(const uint32_t* __restrict__ sp, uint32_t c, Fn&& f) {
    uint32_t s[8];
    bool neg;
    if (!msm_wnaf_words(sp, s, neg)) return;
    const uint32_t half = 1u << (c - 1), mask = (1u << c) - 1;
    uint64_t buf = 0;
    uint32_t nbits = 0, pos = 0, carry = 0, slot = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        buf |= (uint64_t)s[i] << nbits;   // nbits <= 32 here
        nbits += 32;
        if (i < 7) {
            // keep >= 32 bits buffered so that a full window (c <= 22) is always available
            while (nbits > 32) {
                uint64_t tt = carry ? ~buf : buf;
                uint32_t z = tt ? (uint32_t)__builtin_ctzll(tt) : 64u;
                uint32_t room = nbits - 32;
                if (z >= room) {   // only zero digits up to the refill point
                    buf >>= room;
                    pos += room;
                    nbits = 32;
                    break;
                }
                buf >>= z;
                uint32_t val = ((uint32_t)buf & mask) + carry;   // odd
                carry = val > half ? 1u : 0u;
                uint32_t mag = carry ? (1u << c) - val : val;
                f(slot++, pos + z, mag, (carry != 0) != neg);
                buf >>= c;
                pos += z + c;
                nbits -= z + c;
            }
        } else {
            // last word: bits above the buffer are genuine zeros of the scalar
            while (buf != 0 || carry) {
                uint64_t tt = carry ? ~buf : buf;
                uint32_t z = (uint32_t)__builtin_ctzll(tt);   // tt != 0: the top two bits of s are clear
                buf >>= z;
                uint32_t val = ((uint32_t)buf & mask) + carry;
                carry = val > half ? 1u : 0u;
                uint32_t mag = carry ? (1u << c) - val : val;
                f(slot++, pos + z, mag, (carry != 0) != neg);
                buf >>= c;
                pos += z + c;
            }
        }
    }
}

// the recoding over a table with multiples (MsmRecode, msm_types.h)
// f(slot, slice = 255 j + position, odd bucket magnitude in [1, 2^(c-1)), negative), digits in order of increasing position
template <class Fn>
ZK_DI void msm_wnaf_mult(const uint32_t* __restrict__ sp, uint32_t c, const MsmRecode& rc, Fn&& f) {
    uint32_t s[8];
    bool neg;
    if (!msm_wnaf_words(sp, s, neg)) return;
    uint32_t len = 0;   // bits of the value: a wide step needs more than W + 1 of them from its digit on
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (s[i]) len = 32u * i + 32u - (uint32_t)__builtin_clz(s[i]);
    const uint32_t W = c + rc.ext, half = 1u << (c - 1), mask = (1u << c) - 1, maskw = (1u << W) - 1;
    uint64_t buf = 0;
    uint32_t nbits = 0, pos = 0, carry = 0, slot = 0;
    // the digit at position p, the odd residual's low bits at the bottom of buf; returns the bits it consumed
    auto step = [&](uint32_t p) -> uint32_t {
        uint32_t w = c, mag, j = 0;
        if (len > p + W + 1) {
            const uint32_t val = ((uint32_t)buf & maskw) + carry;   // odd, < 2^W
            const uint32_t ch = rc.lut[val >> 1];
            w = c + (ch & 7u);
            j = ch >> 4;
            const uint32_t rho = val & ((1u << w) - 1u), m = 2 * j + 1;
            carry = (ch >> 3) & 1u;
            mag = carry ? (1u << w) - rho : rho;
            uint32_t inv = m;   // m^-1 mod 2^32 (m m = 1 mod 8; every step doubles the bits): the division is exact
#pragma unroll
            for (int it = 0; it < 4; it++) inv *= 2u - m * inv;
            mag *= inv;
        } else {
            const uint32_t val = ((uint32_t)buf & mask) + carry;   // odd
            carry = val > half ? 1u : 0u;
            mag = carry ? (1u << c) - val : val;
        }
        f(slot++, p + MSM_NPOS * j, mag, (carry != 0) != neg);
        return w;
    };
#pragma unroll
    for (int i = 0; i < 8; i++) {
        buf |= (uint64_t)s[i] << nbits;   // nbits <= 32 here
        nbits += 32;
        if (i < 7) {
            // more than 32 bits stay buffered below a digit, so a wide window (c + ext <= 22) is always there
            while (nbits > 32) {
                uint64_t tt = carry ? ~buf : buf;
                uint32_t z = tt ? (uint32_t)__builtin_ctzll(tt) : 64u;
                uint32_t room = nbits - 32;
                if (z >= room) {   // only zero digits up to the refill point
                    buf >>= room;
                    pos += room;
                    nbits = 32;
                    break;
                }
                buf >>= z;
                const uint32_t w = step(pos + z);
                buf >>= w;
                pos += z + w;
                nbits -= z + w;
            }
        } else {
            // last word: bits above the buffer are genuine zeros of the scalar
            while (buf != 0 || carry) {
                uint64_t tt = carry ? ~buf : buf;
                uint32_t z = (uint32_t)__builtin_ctzll(tt);   // tt != 0: the top two bits of s are clear
                buf >>= z;
                const uint32_t w = step(pos + z);
                buf >>= w;
                pos += z + w;
            }
        }
    }
}

// Variable-base mode (no doubling table: bases that are used once).  A scalar is recoded into ODD signed digits at
// FIXED positions - the regular recoding: for odd k, d_i = (k_i mod 2^(w+1)) - 2^w with k_(i+1) = (k_i - d_i) / 2^w,
// which unrolls to k_i = (k >> w i) | 1, so every digit is a function of w + 1 bits of k alone:
//     d_i = (((k >> w i) & (2^(w+1) - 1)) | 1) - 2^w      (i < W - 1),        d_(W-1) = (k >> w (W - 1)) | 1
// with w = c - 1 window bits for the kernels' parameter c (odd magnitudes < 2^w: the same 2^(c-2) buckets and the same
// weights 2 b + 1 as the NAF digits).  An even scalar is replaced by r - s (odd) with every sign flipped.  One job per
// digit position, all over the SAME bases; the host folds the W job results with w doublings between them.
ZK_DI bool msm_vb_digit(const uint32_t* __restrict__ sp, uint32_t c, uint32_t digit, uint32_t n_digits, uint32_t* mag, bool* negative) {
    uint32_t s[9];
    const uint4* q = reinterpret_cast<const uint4*>(sp);
    const uint4 lo = q[0], hi = q[1];
    s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w;
    s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
    s[8] = 0;
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= s[i];
    if (!any) return false;
    const bool flip = (s[0] & 1u) == 0;
    {   // r - s: taken for an even scalar; its borrow / zero result names a NON-CANONICAL scalar (s >= r), which has no digits
        // here (the call fails at its end on the canonical test that runs beside these launches: until then every digit must
        // stay below the 2^w the buckets were sized for - an even s >= r wrapped to ~2^256 and indexed past them)
        uint32_t d[8], bo = 0, co, d_or = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            d[i] = __builtin_subc(MsmConsts::R[i], s[i], bo, &co);
            bo = co;
            d_or |= d[i];
        }
        if (bo || !d_or) return false;
        if (flip) {
#pragma unroll
            for (int i = 0; i < 8; i++) s[i] = d[i];
        }
    }
    const uint32_t w = c - 1, bit = w * digit, word = bit >> 5, sh = bit & 31;
    uint32_t lo_w = 0, hi_w = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {   // no dynamically indexed register array
        if ((uint32_t)i == word) {
            lo_w = s[i];
            hi_w = s[i + 1];
        }
    }
    const uint64_t two = (uint64_t)lo_w | ((uint64_t)hi_w << 32);
    uint32_t t = (uint32_t)(two >> sh);
    if (digit + 1 < n_digits) {
        t = (t & ((2u << w) - 1u)) | 1u;
        const int32_t d = (int32_t)t - (int32_t)(1u << w);
        *mag = (uint32_t)(d < 0 ? -d : d);
        *negative = (d < 0) != flip;
    } else {
        *mag = t | 1u;   // the bits above the last position: < 2^w by the choice of the digit count
        *negative = flip;
    }
    return true;
}
// digits of scalar i of a job, in either mode: f(slot, table slice (the bit position; behind 255 j for multiple j), odd magnitude, negative)
template <class Fn>
ZK_DI void msm_digits(const MsmJob& job, uint32_t i, uint32_t c, const MsmRecode& rc, Fn&& f) {
    if (job.vb_digit == 0) {
        if (rc.lut) msm_wnaf_mult(job.scalars + (size_t)i * 8, c, rc, f);
        else msm_wnaf(job.scalars + (size_t)i * 8, c, f);
    } else {
        uint32_t mag;
        bool negative;
        if (msm_vb_digit(job.scalars + (size_t)i * 8, c, job.vb_digit - 1, job.n_digits, &mag, &negative)) f(0u, 0u, mag, negative);
    }
}

}  // namespace zkdev
