// The derived-point stage behind the wallet's deriving entries (anon_derive.h, elgamal_encrypt.h): a slice of a call as LANES - points
// to decode, multiplications of a decoded point by a scalar, multiplications of G by a scalar, and sums of those brought to affine
// form - through two launches on the library stream, one wave per block, nothing in scratch memory.  The callers describe their
// lanes as data; the only place that knows the stage's buffers and kernels is this header.  Included by anon_derive.h below
// hd_keys.h (fixed_mul and its resident table; wallet_stage.h's point_lane and BoothMul), and by no other unit.
//   k_derive_points    three lane kinds, split at wave boundaries (the first two counts are padded to 64: a wave takes one path)
//       decode         lanes [0, D): point_lane's first kind - read_point + is_prime_order, x | y in Montgomery form and a
//                      zkxt::INTO_XY_* status (~2 800 dependent products).  One per DISTINCT encoding of the slice (Encodings).
//       variable       point_lane's second kind with BoothMul: [scalar] point over signed fixed windows of 3 bits, all lanes adding
//                      at the same 85 positions (~3 350 with read_point).  The scalar is one of the slice's POOL, named by the
//                      lane's index word: lanes that share a scalar read one copy of it.
//       fixed          a descriptor of four words per lane: the pool index of the scalar (NONE: a padding lane, which returns), the
//                      windows hd_keys.h fixed_mul walks over the resident positional table (43, or as few as the scalar can
//                      occupy; ~7 products each), a table entry to add afterwards (ext_add_affine; or NONE), the lane's slot in proj.
//                      A caller whose lanes differ in their windows pads between them to 64: no wave waits for its longest lane.
//                      The variable and fixed lanes leave X Y Z T.  LDS is k_keys_points': 17 slots x 32 x 64 = 34 816 B.
//   k_derive_combine   one lane per output point: a source slot (+ an addend slot, its x and T negated on request), one inversion
//                      (pow_windows, ~330), Point::write's bytes and - where a lane's output is 24 words - x | y in Montgomery
//                      form.  A source that names a decode lane takes that lane's status for its own, and 32 zero bytes where it
//                      is a refusal.  LDS: pow_windows' 16 slots, 32 768 B.
//   The lane bodies are the sibling kernels' (point_lane, BoothMul, fixed_mul, unchanged): the stage costs no new arithmetic, keeps
//   their LDS budget and no scratch (tests/test_anon_derive.py reads both off the code object; DESIGN.md 4.10.5 has the figures).
// Secrets: the pool, the projective points and everything derived from them live in the Stage's DevBufs, zeroed before they are
// released (zk_memory_stats counts them), on success and on every failure; its host copy of the upload is wiped on every way out and
// before it may move.  The stage is NOT constant-time: a zero digit of a lane's scalar skips that lane's addition.
#pragma once
#include "hd_keys.h"

namespace zkstage {

using zkdev::Fr;
using zkxt::EP;
using zkxt::Lds;

constexpr uint32_t NONE = 0xffffffffu;
static_assert(zkhd::SLOT_SCALAR == zkscan::KEYS_SLOT_SCALAR && zkhd::LDS_WORDS * 4 == zkscan::KEYS_LDS_BYTES && zkscan::KEYS_LDS_BYTES <= 36864,
              "one LDS layout for the three lane kinds, in k_rj_check's budget");

// ---- device
ZK_DI EP ld_ep(const uint32_t* p) { return EP{zkrj::ld_fr(p), zkrj::ld_fr(p + 8), zkrj::ld_fr(p + 16), zkrj::ld_fr(p + 24)}; }
// enc: d64 x 8 words (n_dec used).  venc, vidx: n_var x 8 words and n_var words, a lane's base and the pool index of its scalar.
// tab: zkhd::TAB_WORDS.  pool: 8 plain words per scalar.  fix: n_fix descriptors (above); addends: table entries, 24 words each.
// xy: n_dec x 16 words, status: n_dec words (point_lane's).  proj: 32 words per slot, X Y Z T - the variable lanes' [0, n_var) first.
static __global__ void __launch_bounds__(64)
k_derive_points(const uint32_t* enc, uint32_t n_dec, uint32_t d64, const uint32_t* venc, const uint32_t* vidx, uint32_t n_var, uint32_t v64,
                const uint32_t* tab, const uint32_t* pool, const uint4* fix, const uint32_t* addends, uint32_t n_fix, uint32_t* xy, uint32_t* status,
                uint32_t* proj) {
    ZK_SHARED uint32_t table[zkscan::KEYS_LDS_SLOTS * 8 * 64];
    const Lds L{table + threadIdx.x};
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t < d64 + v64) {
        const auto pool_mul = [=](const Lds& l, uint32_t r, const Fr& xm, const Fr& ym, const Fr& d2) { return zkscan::BoothMul{pool}(l, vidx[r], xm, ym, d2); };
        zkscan::point_lane(L, enc, n_dec, d64, venc, n_var, pool_mul, xy, status, proj);
        return;
    }
    const uint32_t f = t - d64 - v64;
    if (f >= n_fix) return;
    const uint4 d = fix[f];
    if (d.x == NONE) return;
    L.st(zkhd::SLOT_SCALAR, zkrj::ld_fr(pool + (size_t)d.x * 8));
    EP p = zkhd::fixed_mul<false>(L, tab, nullptr, d.y);
    if (d.z != NONE) {
        const uint32_t* a = addends + (size_t)d.z * zkhd::ENTRY_WORDS;
        p = zkrj::ext_add_affine(p, zkrj::ld_fr(a), zkrj::ld_fr(a + 8), zkrj::ld_fr(a + 16), false, true);
    }
    uint32_t* o = proj + (size_t)d.w * 32;
    zkscan::st_fr(o, p.X);
    zkscan::st_fr(o + 8, p.Y);
    zkscan::st_fr(o + 16, p.Z);
    zkscan::st_fr(o + 24, p.T);
}
// src: n x 4 words - the lane's source in proj, its addend there (or NONE), whether the addend is negated, the decode lane it
// answers for (or NONE).  dstatus: k_derive_points' status.  out: n x out_words words (8 or 24) - Point::write, zero where the
// decode lane is a refusal, then x | y in Montgomery form where there is room.  status (or NULL): n words.
// (Z is never zero where the points are accepted: the addition law is complete on prime-order points.)
static __global__ void __launch_bounds__(64)
k_derive_combine(const uint32_t* proj, const uint32_t* dstatus, const uint4* src, uint32_t n, uint32_t out_words, uint32_t* out, uint32_t* status) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Lds L{table + threadIdx.x};
    const uint4 s = src[t];
    const uint32_t st = s.w == NONE ? (uint32_t)zkxt::INTO_XY_OK : dstatus[s.w];
    if (status) status[t] = st;
    uint32_t* o = out + (size_t)t * out_words;
    if (st != zkxt::INTO_XY_OK) {
        zkscan::st_fr(o, Fr::zero());
        return;
    }
    EP p = ld_ep(proj + (size_t)s.x * 32);
    if (s.y != NONE) {
        EP q = ld_ep(proj + (size_t)s.y * 32);
        if (s.z) {
            q.X = neg(q.X);
            q.T = neg(q.T);
        }
        p = zkxt::ext_add(p, q, zkxt::jubjub_d2());
    }
    constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
    const Fr zi = zkxt::pow_windows(L, p.Z, EI);
    const Fr x = mul(p.X, zi), y = mul(p.Y, zi);
    zkscan::st_fr(o, zkxt::point_words(x, y));
    if (out_words == 24) {
        zkscan::st_fr(o + 8, x);
        zkscan::st_fr(o + 16, y);
    }
}

// ---- host side
// the distinct 32-byte encodings of a slice, in the order they are first met
struct Encodings {
    std::vector<uint32_t> cell;   // index + 1; 0 = empty
    std::vector<uint8_t> enc;
    size_t mask;
    explicit Encodings(size_t expected) {
        size_t cap = 16;
        while (cap < 2 * expected + 2) cap <<= 1;
        cell.assign(cap, 0);
        mask = cap - 1;
        enc.reserve(expected * 32);
    }
    size_t size() const { return enc.size() / 32; }
    uint32_t put(const uint8_t* b) {
        uint64_t w[4];
        memcpy(w, b, 32);
        uint64_t h = w[0] * 0x9e3779b97f4a7c15ull;
        h = ((h ^ (h >> 29)) + w[1]) * 0xbf58476d1ce4e5b9ull;
        h = ((h ^ (h >> 31)) + w[2]) * 0x94d049bb133111ebull;
        h = ((h ^ (h >> 30)) + w[3]) * 0x9e3779b97f4a7c15ull;
        for (size_t at = (h ^ (h >> 32)) & mask;; at = (at + 1) & mask) {
            const uint32_t c = cell[at];
            if (c && !memcmp(&enc[(size_t)(c - 1) * 32], b, 32)) return c - 1;
            if (!c) {
                enc.insert(enc.end(), b, b + 32);
                return (cell[at] = (uint32_t)size()) - 1;
            }
        }
    }
};

// A slice as its caller describes it.  The counts first; begin() lays the upload out and the caller fills the regions in place.
struct Shape {
    size_t dec, var, pool, fix, addends, out;   // distinct encodings | variable lanes | scalars | fixed lanes, padding included | entries | combine lanes
    uint32_t out_words;                         // per combine lane: 8, or 24 with x | y
    bool statuses;   // the combine answers for decode lanes and a status per output comes back; otherwise xy and the decode statuses do
    const char *upload, *points, *combine, *download;   // the ProfScope names
};
// One per call, around its slice loop.  Between begin() and run(): enc (dec x 8 words), venc (var x 8) and vidx (var), pool (pool x
// 8), addends (addends x 24), fix (fix x 4, every lane empty until it is written: slot w is var + a number below `fix`), src (out x 4).
// After run(): out (out x out_words) and either status (out) or xy (dec x 16) and dstatus (dec).
struct Stage {
    zkrt::DevBuf din, dout;             // scalars and their multiples: zeroed before they go back, on every way out of the caller
    std::vector<uint32_t> hin, back;    // hin: the slice as it is uploaded, scalars among it; back: bytes, coordinates, statuses - public
    Shape s{};
    uint32_t *enc = nullptr, *venc = nullptr, *vidx = nullptr, *pool = nullptr, *addends = nullptr, *fix = nullptr, *src = nullptr;
    const uint32_t *out = nullptr, *status = nullptr, *xy = nullptr, *dstatus = nullptr;
    static size_t pad(size_t v, size_t to) { return (v + to - 1) / to * to; }
    void wipe() {
        if (!hin.empty()) explicit_bzero(hin.data(), hin.size() * 4);
    }
    ~Stage() { wipe(); }
    void begin(const Shape& shape) {
        s = shape;
        wipe();   // (before assign() may move it)
        // in: encodings | bases | scalars | entries | descriptors | combine sources | pool indices
        hin.assign(pad(s.dec, 64) * 8 + s.var * 8 + s.pool * 8 + s.addends * zkhd::ENTRY_WORDS + s.fix * 4 + s.out * 4 + s.var, 0);
        enc = hin.data(), venc = enc + pad(s.dec, 64) * 8, pool = venc + s.var * 8, addends = pool + s.pool * 8;
        fix = addends + s.addends * zkhd::ENTRY_WORDS, src = fix + s.fix * 4, vidx = src + s.out * 4;
        memset(fix, 0xff, s.fix * 16);
    }
    zk_status run(const uint32_t* tab) {
        const size_t d64 = pad(s.dec, 64), v64 = pad(s.var, 64);
        // out: the combine's output | its statuses (padded to 4) || the decode lanes' statuses (padded to 4) | their coordinates ||
        // the projective points.  What comes back ends at the first || with statuses, at the second without.
        const size_t w_st = s.out * s.out_words, w_dst = w_st + (s.statuses ? pad(s.out, 4) : 0), w_xy = w_dst + pad(s.dec, 4), w_proj = w_xy + s.dec * 16,
                     back_words = s.statuses ? w_dst : w_proj;
        back.resize(std::max(back.size(), back_words));
        ZK_TRY(din.ensure(hin.size() * 4));
        ZK_TRY(dout.ensure((w_proj + (s.var + s.fix) * 32) * 4));
        const uint32_t* d_in = din.as<const uint32_t>();
        uint32_t* d_out = dout.as<uint32_t>();
        {
            zkrt::ProfScope ps(s.upload);
            HIP_TRY(hipMemcpyAsync(din.p, hin.data(), hin.size() * 4, hipMemcpyHostToDevice, zkrt::g_stream));
        }
        {
            zkrt::ProfScope ps(s.points);
            ZK_LAUNCH(k_derive_points, dim3((unsigned)((d64 + v64 + pad(s.fix, 64)) / 64)), dim3(64), 0, zkrt::g_stream, d_in, (uint32_t)s.dec, (uint32_t)d64,
                      d_in + (venc - enc), d_in + (vidx - enc), (uint32_t)s.var, (uint32_t)v64, tab, d_in + (pool - enc),
                      reinterpret_cast<const uint4*>(d_in + (fix - enc)), d_in + (addends - enc), (uint32_t)s.fix, d_out + w_xy, d_out + w_dst, d_out + w_proj);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps(s.combine);
            ZK_LAUNCH(k_derive_combine, dim3((unsigned)((s.out + 63) / 64)), dim3(64), 0, zkrt::g_stream, d_out + w_proj, d_out + w_dst,
                      reinterpret_cast<const uint4*>(d_in + (src - enc)), (uint32_t)s.out, s.out_words, d_out, s.statuses ? d_out + w_st : nullptr);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps(s.download);
            HIP_TRY(hipMemcpyAsync(back.data(), dout.p, back_words * 4, hipMemcpyDeviceToHost, zkrt::g_stream));
        }
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        out = back.data(), status = back.data() + w_st, dstatus = back.data() + w_dst, xy = back.data() + w_xy;
        return ZK_OK;
    }
};

}  // namespace zkstage
