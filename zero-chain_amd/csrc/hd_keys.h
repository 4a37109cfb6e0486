// Hierarchical key derivation (zface/src/derive/mod.rs, a ZIP32-style scheme): the children of one extended key - an extended
// spending key (xsk) or its watch-only half, an extended proof generation key (xpgk) - with the account of each (decryption key,
// encryption key: core/proofs/src/no_std_aliases/keys.rs:166-198), in one call (zk_hd_master, zk_hd_xpgk_from_xsk, zk_hd_derive,
// zk_scan_keys_create_hd, zk_jubjub_base_mul_dev).  Included by wallet.cpp below scan_keys.h, and by no other unit.
//
//   xkey     depth (1) | parent_enckey_tag (4) | child_index (u32 LE) | chain_code (32) | key (32): 73 bytes      mod.rs:125-134, 219-228
//   I        prf_expand_vec(chain_code, [0x11], sk, i LE) for a hardened child (xsk only), else (.., [0x12], pgk, i LE)   mod.rs:69-86, 165-178
//   f        Fs::to_uniform(prf_expand(I[0..32], [0x13])); the child's chain code is I[32..64]                      mod.rs:94, 186
//   child    sk + f (xsk) or [f]G + pgk (xpgk); tag = BLAKE2b-256("ZerochainEFinger", parent pgk)[0..4]             mod.rs:92-103, 184-196
//   account  dk = BLAKE2s-256("zech_bdk", child pgk) with the top five bits cleared, enc_key = [dk]G               keys.rs:166-198
// G is FixedGenerators::NoteCommitmentRandomness, the generator of zkwit::tables().
//
// The hashes (two BLAKE2b per child, the tag, to_uniform, sk + f) run on the zk_set_host_threads pool.  The point work - per child
// [f]G + pgk and [dk]G, two inversions, two encodings - has two forms that write the same bytes:
//   host    jubjub_fixed_mul_ext and one batch_to_affine per thread and stage
//   device  k_hd_children, one lane per child, one wave per block, nothing in scratch memory.  ONE route for both kinds: the device
//           receives f_i and the parent's pgk, never a spending key ([f]G + [sk]G is the pgk of sk + f).
//     fixed_mul   a multiplication by G alone needs no doublings: a positional table holds k 2^(6w) G for the 43 six-bit windows w
//                 and k = 1 .. 32 as (y + x, y - x, 2 d x y) in Montgomery form (gtable()'s entry format; 43 x 32 x 96 B = 132 096 B,
//                 built on the host once, uploaded once per device and kept - public data).  The lane walks the 43 signed digits
//                 of its scalar (zkrj::booth_digit<6>; window 42 holds only the carry) and adds the window's entry where the digit
//                 is not zero (ext_add_affine, 7 products with T): about 300 dependent products instead of the 2 300 of a chain
//                 with doublings.  All 64 lanes add at the same 43 positions.
//     lane        fixed_mul(f) + pgk, 1 / Z (pow_windows, ~330), Point::write, BLAKE2s in the lane (one block, one compression,
//                 the message schedule spelled out so that nothing is indexed at run time), the mask, fixed_mul(dk), 1 / Z,
//                 Point::write: about 1 300 dependent products, 96 bytes out.
//     LDS         [slot][word][lane]: slots 1 .. 15 pow_windows' powers, slot 16 the scalar's eight words (dynamic indexing of
//                 registers would go to scratch) = 17 x 32 x 64 = 34 816 B; the staged form adds one window's 32 entries, 3 072 B.
//     table read  each lane loads its own 96-byte entry from global memory, as k_rj_check does; or (ZKAMD_HD_STAGE_TABLE=1) the
//                 block first copies the window's 32 entries into LDS, between two barriers.  Measured (profiles/r24_hd_probe.json): the
//                 kernel takes 0.90 ms with the lanes' own loads and 0.93 ms staged, at every size from 64 to 4096 lanes - the
//                 lanes' own loads are the default.
//   k_base_mul  the same fixed_mul with chosen scalars and an optional addend (read_point, no subgroup test): zk_jubjub_base_mul_dev.
// Secrets: f_i, dk_i and the child spending keys are key-derived.  The device buffers that hold them live for one call and are
// zeroed before they are returned (DevBuf, counted by zk_memory_stats), on success and on failure; host copies are wiped on every
// way out.  The device form is NOT constant-time: a zero digit skips its addition.
#pragma once
#include "scan_keys.h"
#include <map>
#include <mutex>

namespace zkhd {

using zkdev::Fr;
using zkrt::fail;
using zkxt::EP;
using zkxt::Lds;

// ZKAMD_HD_HOST_MAX: children up to which the host form runs (read per call; 0 = always the kernel).  Measured (profiles/r24_hd_probe.json,
// 16 host threads, all three outputs): the kernel is 0.90 ms from 64 to 4096 lanes and the device form 1.52 ms at 64 children, 1.55 at
// 256 and 1.59 at 1024 (the hashes and the buffers beside the kernel), the host form 1.11 ms at 64, 1.46 at 256 and 3.01 at 1024 - 256
// is the largest probed size at which the host form is still the faster one.
constexpr size_t HOST_MAX = 256;
constexpr int WINDOW = 6, WINDOWS = 252 / WINDOW + 1, MULTIPLES = 1 << (WINDOW - 1);
constexpr uint32_t ENTRY_WORDS = 24, WINDOW_WORDS = MULTIPLES * ENTRY_WORDS, TAB_WORDS = WINDOWS * WINDOW_WORDS;
constexpr uint32_t SLOT_SCALAR = 16, LDS_SLOTS = 17, LDS_WORDS = LDS_SLOTS * 8 * 64;
static_assert(252 % WINDOW == 0 && WINDOWS == 43 && TAB_WORDS * 4 == 132096, "43 windows of 32 entries; the one at bit 252 holds the carry");
static_assert((LDS_WORDS + WINDOW_WORDS) * 4 <= 65536, "both forms within a block's 64 KB");
constexpr size_t XKEY_BYTES = ZK_HD_XKEY_BYTES;
constexpr size_t SLICE = (size_t)1 << 20;   // lanes per launch

// ---- device
// [scalar in SLOT_SCALAR] G, extended with T.  tab: TAB_WORDS.  STAGED: every lane of the block takes part (two barriers per window).
// windows: how many the scalar can occupy, its top digit's carry included (elgamal_encrypt.h: 6 for a 32-bit value).
template <bool STAGED>
ZK_DI EP fixed_mul(const Lds& L, const uint32_t* tab, uint32_t* stage, uint32_t windows = (uint32_t)WINDOWS) {
    EP acc = zkxt::ep_neutral();
#pragma unroll 1
    for (uint32_t w = 0; w < windows; w++) {
        const uint32_t* win = tab + (size_t)w * WINDOW_WORDS;
        if constexpr (STAGED) {
            __syncthreads();   // the readers of the window before are done
            for (uint32_t k = threadIdx.x; k < WINDOW_WORDS / 4; k += 64) reinterpret_cast<uint4*>(stage)[k] = reinterpret_cast<const uint4*>(win)[k];
            __syncthreads();
        }
        const int d = zkrj::booth_digit<WINDOW>(L, SLOT_SCALAR, (uint32_t)WINDOW * w);
        if (d) {
            const uint32_t* e = (STAGED ? stage : win) + (uint32_t)((d < 0 ? -d : d) - 1) * ENTRY_WORDS;
            acc = zkrj::ext_add_affine(acc, zkrj::ld_fr(e), zkrj::ld_fr(e + 8), zkrj::ld_fr(e + 16), d < 0, true);
        }
    }
    return acc;
}
// Point::write of a projective point, as 8 words: one inversion (Z is never zero: the addition law is complete on this curve)
ZK_DI Fr affine_words(const Lds& L, const EP& p) {
    constexpr zkxt::PowDigits EI = zkxt::digits_inverse();
    const Fr zi = zkxt::pow_windows(L, p.Z, EI);
    return zkxt::point_words(mul(p.X, zi), mul(p.Y, zi));
}
// BLAKE2s-256 personalised "zech_bdk" of the 32 bytes in m (keys.rs:166-175): one block, one compression.  Every index is a
// constant: the state and the message stay in registers.
ZK_DI uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
#define ZKHD_G(a, b, c, d, x, y)          \
    do {                                  \
        a = a + b + (x);                  \
        d = rotr32(d ^ a, 16);            \
        c = c + d;                        \
        b = rotr32(b ^ c, 12);            \
        a = a + b + (y);                  \
        d = rotr32(d ^ a, 8);             \
        c = c + d;                        \
        b = rotr32(b ^ c, 7);             \
    } while (0)
// (words 8 .. 15 of the block are zero: M(i) is m.l[i] below 8)
#define ZKHD_M(i) ((i) < 8 ? m.l[(i) & 7] : 0u)
#define ZKHD_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                                 \
        ZKHD_G(v0, v4, v8, v12, ZKHD_M(s0), ZKHD_M(s1));                                 \
        ZKHD_G(v1, v5, v9, v13, ZKHD_M(s2), ZKHD_M(s3));                                 \
        ZKHD_G(v2, v6, v10, v14, ZKHD_M(s4), ZKHD_M(s5));                                \
        ZKHD_G(v3, v7, v11, v15, ZKHD_M(s6), ZKHD_M(s7));                                \
        ZKHD_G(v0, v5, v10, v15, ZKHD_M(s8), ZKHD_M(s9));                                \
        ZKHD_G(v1, v6, v11, v12, ZKHD_M(s10), ZKHD_M(s11));                              \
        ZKHD_G(v2, v7, v8, v13, ZKHD_M(s12), ZKHD_M(s13));                               \
        ZKHD_G(v3, v4, v9, v14, ZKHD_M(s14), ZKHD_M(s15));                               \
    } while (0)
ZK_DI Fr blake2s_bdk(const Fr& m) {
    constexpr uint32_t IV0 = 0x6A09E667u, IV1 = 0xBB67AE85u, IV2 = 0x3C6EF372u, IV3 = 0xA54FF53Au, IV4 = 0x510E527Fu, IV5 = 0x9B05688Cu,
                       IV6 = 0x1F83D9ABu, IV7 = 0x5BE0CD19u;
    // the parameter block: digest length 32, fanout 1, depth 1; "zech" "_bdk" in words 6 and 7
    constexpr uint32_t H0 = IV0 ^ 0x01010020u, H6 = IV6 ^ 0x6863657au, H7 = IV7 ^ 0x6b64625fu;
    uint32_t v0 = H0, v1 = IV1, v2 = IV2, v3 = IV3, v4 = IV4, v5 = IV5, v6 = H6, v7 = H7;
    uint32_t v8 = IV0, v9 = IV1, v10 = IV2, v11 = IV3, v12 = IV4 ^ 32u, v13 = IV5, v14 = ~IV6, v15 = IV7;   // 32 bytes in, the last block
    ZKHD_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    ZKHD_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    ZKHD_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    ZKHD_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    ZKHD_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    ZKHD_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    ZKHD_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    ZKHD_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    ZKHD_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    ZKHD_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    Fr h;
    h.l[0] = H0 ^ v0 ^ v8;
    h.l[1] = IV1 ^ v1 ^ v9;
    h.l[2] = IV2 ^ v2 ^ v10;
    h.l[3] = IV3 ^ v3 ^ v11;
    h.l[4] = IV4 ^ v4 ^ v12;
    h.l[5] = IV5 ^ v5 ^ v13;
    h.l[6] = H6 ^ v6 ^ v14;
    h.l[7] = H7 ^ v7 ^ v15;
    return h;
}
#undef ZKHD_ROUND
#undef ZKHD_M
#undef ZKHD_G

// tab: TAB_WORDS.  parent: 24 words, the parent's pgk as a table entry.  f: n x 8 plain words.  out: n x 24 words - the child's
// pgk (Point::write), dk, the encryption key (Point::write).
template <bool STAGED>
static __global__ void __launch_bounds__(64)
k_hd_children(const uint32_t* tab, const uint32_t* parent, const uint32_t* f, uint32_t* out, uint32_t n) {
    ZK_SHARED uint32_t table[LDS_WORDS + (STAGED ? WINDOW_WORDS : 0)];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    const bool live = t < n;
    if (!STAGED && !live) return;   // (the staged form keeps every lane for its barriers: a lane past the end multiplies by zero)
    const Lds L{table + threadIdx.x};
    uint32_t* stage = table + (STAGED ? LDS_WORDS : 0);
    L.st(SLOT_SCALAR, live ? zkrj::ld_fr(f + (size_t)t * 8) : Fr::zero());
    EP p = fixed_mul<STAGED>(L, tab, stage);
    p = zkrj::ext_add_affine(p, zkrj::ld_fr(parent), zkrj::ld_fr(parent + 8), zkrj::ld_fr(parent + 16), false, false);
    const Fr pgk = affine_words(L, p);
    Fr dk = blake2s_bdk(pgk);
    dk.l[7] &= 0x07ffffffu;   // byte 31 &= 0b0000_0111
    L.st(SLOT_SCALAR, dk);
    const Fr enc = affine_words(L, fixed_mul<STAGED>(L, tab, stage));
    if (!live) return;
    uint32_t* o = out + (size_t)t * 24;
    zkscan::st_fr(o, pgk);
    zkscan::st_fr(o + 8, dk);
    zkscan::st_fr(o + 16, enc);
}
// scalars: n x 8 plain words.  addends: n x 8 words (Point::write encodings) or NULL.  points: n x 8 words, [scalar] G (+ addend),
// zero where the addend is refused.  status: n words, zkxt::INTO_XY_* of the addend (not written without addends).
template <bool STAGED>
static __global__ void __launch_bounds__(64)
k_base_mul(const uint32_t* tab, const uint32_t* scalars, const uint32_t* addends, uint32_t* points, uint32_t* status, uint32_t n) {
    ZK_SHARED uint32_t table[LDS_WORDS + (STAGED ? WINDOW_WORDS : 0)];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    const bool live = t < n;
    if (!STAGED && !live) return;
    const Lds L{table + threadIdx.x};
    uint32_t* stage = table + (STAGED ? LDS_WORDS : 0);
    uint32_t st = zkxt::INTO_XY_OK;
    Fr x = Fr::zero(), y, xm = Fr::zero(), ym = Fr::zero(), d = Fr::zero();
    if (addends && live) st = zkxt::read_point(L, addends + (size_t)t * 8, &x, &y, &xm, &ym, &d);
    L.st(SLOT_SCALAR, live ? zkrj::ld_fr(scalars + (size_t)t * 8) : Fr::zero());
    EP p = fixed_mul<STAGED>(L, tab, stage);
    if (addends && live && st == zkxt::INTO_XY_OK) p = zkrj::ext_add_affine(p, add(ym, xm), sub(ym, xm), mul(mul(xm, ym), dbl(d)), false, false);
    const Fr w = affine_words(L, p);
    if (!live) return;
    zkscan::st_fr(points + (size_t)t * 8, st == zkxt::INTO_XY_OK ? w : Fr::zero());
    if (addends) status[t] = st;
}

// ---- host side: the table
// k 2^(6 w) G for w = 0 .. 42, k = 1 .. 32, as the kernels read them; built once per process
inline const std::vector<uint32_t>& host_table() {
    static const std::vector<uint32_t> tab = [] {
        std::vector<zkwit::EPoint> proj((size_t)WINDOWS * MULTIPLES);
        zkwit::EPoint base = zkwit::to_ext(zkwit::tables().win[0][1]);
        for (int w = 0; w < WINDOWS; w++) {
            zkwit::EPoint* m = &proj[(size_t)w * MULTIPLES];
            m[0] = base;
            for (int k = 1; k < MULTIPLES; k++) m[k] = zkwit::ext_add(m[k - 1], base);
            base = zkwit::ext_add(m[MULTIPLES - 1], m[MULTIPLES - 1]);   // 64 times: the next window's unit
        }
        std::vector<zkwit::JPoint> aff(proj.size());
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        std::vector<uint32_t> w(TAB_WORDS);
        const zkhost::Fr d2 = zkwit::edwards_d().dbl();
        for (size_t i = 0; i < aff.size(); i++) {
            const zkhost::Fr e[3] = {aff[i].y + aff[i].x, aff[i].y - aff[i].x, aff[i].x * aff[i].y * d2};
            memcpy(&w[ENTRY_WORDS * i], e, 96);
        }
        return w;
    }();
    return tab;
}
// ... and per device, uploaded on the first call that runs a kernel there and kept for the process (public: freed without a wipe,
// and like the stream contexts of host_common.h never torn down)
inline zk_status device_table(int device, const uint32_t** out) {
    static std::mutex mu;
    static std::map<int, zkrt::DevBuf*> tabs;
    const std::vector<uint32_t>& host = host_table();
    std::lock_guard<std::mutex> lock(mu);
    zkrt::DevBuf*& b = tabs[device];
    if (!b) {
        std::unique_ptr<zkrt::DevBuf> fresh(new zkrt::DevBuf());
        fresh->is_public = true;
        const zk_status rc = fresh->upload(host);
        if (rc != ZK_OK) {
            tabs.erase(device);
            return rc;
        }
        b = fresh.release();
    }
    *out = b->as<uint32_t>();
    return ZK_OK;
}
inline size_t host_max() {
    const char* e = getenv("ZKAMD_HD_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : HOST_MAX;
}
// ZKAMD_HD_STAGE_TABLE=1: the kernels copy each window of the table into LDS first (read per call; default: every lane loads its own entry)
inline bool stage_table() {
    const char* e = getenv("ZKAMD_HD_STAGE_TABLE");
    return e && *e && atoi(e) != 0;
}
template <class Plain, class Staged, class... Args>
inline void launch_form(bool staged, Plain plain, Staged with_stage, size_t lanes, Args... args) {
    const dim3 grid((unsigned)((lanes + 63) / 64)), block(64);
    if (staged) {
        ZK_LAUNCH_SYNC(with_stage, grid, block, 0, zkrt::g_stream, args...);
    } else {
        ZK_LAUNCH(plain, grid, block, 0, zkrt::g_stream, args...);
    }
}

// ---- host side: the hashes
constexpr uint8_t EXPAND_PERSON[16] = {'z', 'e', 'c', 'h', '_', 'E', 'x', 'p', 'a', 'n', 'd', 'S', 'e', 'e', 'd', '_'};
constexpr uint8_t MASTER_PERSON[16] = {'Z', 'e', 'r', 'o', 'c', 'h', 'a', 'i', 'n', '_', 'M', 'a', 's', 't', 'e', 'r'};
constexpr uint8_t FINGER_PERSON[16] = {'Z', 'e', 'r', 'o', 'c', 'h', 'a', 'i', 'n', 'E', 'F', 'i', 'n', 'g', 'e', 'r'};
constexpr uint8_t BDK_PERSON[8] = {'z', 'e', 'c', 'h', '_', 'b', 'd', 'k'};
constexpr size_t OFF_TAG = 1, OFF_INDEX = 5, OFF_CHAIN = 9, OFF_KEY = 41;

// Fs::to_uniform(BLAKE2b-512("zech_ExpandSeed_", a || b)): SpendingKey::from_seed with b empty, prf_expand with b = [t]
inline void expand_to_fs(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint64_t out[4]) {
    zkhash::Blake2b h(EXPAND_PERSON);
    uint8_t d[64];
    WipeOnExit wipe_h{&h, sizeof(h)}, wipe_d{d, sizeof(d)};
    h.update(a, a_len);
    h.update(b, b_len);
    h.finish(d);
    fs_to_uniform(d, 64, out);
}
// ProofGenerationKey::into_decryption_key of the 32 bytes of a pgk: plain words
inline void dec_key_of(const uint8_t pgk[32], uint64_t out[4]) {
    zkhash::Blake2s h(BDK_PERSON);
    uint8_t d[32];
    WipeOnExit wipe_h{&h, sizeof(h)}, wipe_d{d, sizeof(d)};
    h.update(pgk, 32);
    h.finish(d);
    d[31] &= 0x07;
    zkrt::load_scalar_le(d, out);
}

// an extended key as the entries read it: ExtendedSpendingKey::read / ExtendedProofGenerationKey::read
struct Parent {
    uint8_t depth = 0, chain[32], sk_bytes[32], pgk_bytes[32], tag[4];   // tag: of THIS key, what its children carry
    uint64_t sk[4] = {0, 0, 0, 0};                                     // (xsk only)
    zkwit::JPoint pgk;
    ~Parent() {
        explicit_bzero(sk, sizeof(sk));
        explicit_bzero(sk_bytes, sizeof(sk_bytes));
    }
};
inline zk_status check_kind(uint32_t kind) {
    return kind == ZK_HD_XSK || kind == ZK_HD_XPGK ? ZK_OK : fail(ZK_ERR_INVALID_ARGUMENT, "kind must be ZK_HD_XSK or ZK_HD_XPGK");
}
inline zk_status parent_read(uint32_t kind, const uint8_t* xkey, Parent* p) {
    p->depth = xkey[0];
    memcpy(p->chain, xkey + OFF_CHAIN, 32);
    if (kind == ZK_HD_XSK) {
        memcpy(p->sk_bytes, xkey + OFF_KEY, 32);
        zkrt::load_scalar_le(p->sk_bytes, p->sk);
        if (!fs_lt_mod(p->sk)) return fail(ZK_ERR_INVALID_ARGUMENT, "xsk: the spending key is not a canonical Fs scalar");   // SpendingKey::read
        p->pgk = jubjub_fixed_mul(p->sk);
    } else {
        ZK_TRY(decode_prime_order(xkey + OFF_KEY, &p->pgk, "xpgk: the proof generation key"));   // ProofGenerationKey::read
    }
    jubjub_encode(p->pgk.x, p->pgk.y, p->pgk_bytes);   // into_bytes: the canonical bytes, whatever came
    zkhash::Blake2b h(FINGER_PERSON, 32);   // EncKeyFingerPrint
    uint8_t d[64];
    h.update(p->pgk_bytes, 32);
    h.finish(d);
    memcpy(p->tag, d, 4);
    return ZK_OK;
}
inline void xkey_write(uint8_t* out, unsigned depth, const uint8_t tag[4], uint32_t index, const uint8_t chain[32], const uint8_t key[32]) {
    out[0] = (uint8_t)depth;
    memcpy(out + OFF_TAG, tag, 4);
    for (int j = 0; j < 4; j++) out[OFF_INDEX + j] = (uint8_t)(index >> (8 * j));
    memcpy(out + OFF_CHAIN, chain, 32);
    memcpy(out + OFF_KEY, key, 32);
}

// what the children of one call are made of; every array n x 32 bytes.  f, dk and the child spending keys are wiped on the way out
struct Children {
    std::vector<uint64_t> f, sk, dk;
    std::vector<uint8_t> chain, pgk, enc;
    ~Children() {
        for (std::vector<uint64_t>* v : {&f, &sk, &dk})
            if (!v->empty()) explicit_bzero(v->data(), v->size() * sizeof(uint64_t));
    }
};
inline zk_status check_indices(uint32_t kind, const Parent& p, const uint32_t* indices, size_t n) {
    if (p.depth == 255) return fail(ZK_ERR_INVALID_ARGUMENT, "the parent's depth is 255: a child's depth does not fit its byte");
    for (size_t i = 0; kind == ZK_HD_XPGK && i < n; i++)
        if (indices[i] >> 31)
            return fail(ZK_ERR_INVALID_ARGUMENT, "index " + std::to_string(i) + " (" + std::to_string(indices[i]) +
                                                     ") is hardened: an extended proof generation key derives non-hardened children only");
    return ZK_OK;
}
inline zk_status hash_children(uint32_t kind, const Parent& p, const uint32_t* indices, size_t n, Children* c) {
    c->f.resize(n * 4);
    c->chain.resize(n * 32);
    if (kind == ZK_HD_XSK) c->sk.resize(n * 4);
    return zkrt::for_each_status(n, 64, [&](size_t i) -> zk_status {
        const uint32_t index = indices[i];
        const bool hardened = (index >> 31) != 0;
        const uint8_t domain = hardened ? 0x11 : 0x12, i_le[4] = {(uint8_t)index, (uint8_t)(index >> 8), (uint8_t)(index >> 16), (uint8_t)(index >> 24)};
        zkhash::Blake2b h(EXPAND_PERSON);
        uint8_t d[64];
        WipeOnExit wipe_h{&h, sizeof(h)}, wipe_d{d, sizeof(d)};
        h.update(p.chain, 32);
        h.update(&domain, 1);
        h.update(hardened ? p.sk_bytes : p.pgk_bytes, 32);
        h.update(i_le, 4);
        h.finish(d);
        const uint8_t t13 = 0x13;
        expand_to_fs(d, 32, &t13, 1, &c->f[4 * i]);
        memcpy(&c->chain[32 * i], d + 32, 32);
        if (kind == ZK_HD_XSK) fs_add(p.sk, &c->f[4 * i], &c->sk[4 * i]);
        return ZK_OK;
    });
}

// ---- host side: the point work.  c->pgk, c->dk and (want_enc) c->enc from c->f and the parent's pgk.
inline zk_status points_host(const Parent& p, size_t n, bool want_enc, Children* c) {
    (void)zkwit::tables();
    const zkwit::EPoint parent = zkwit::to_ext(p.pgk);
    return zkrt::for_each_range(n, 64, [&](size_t i0, size_t i1) -> zk_status {
        std::vector<zkwit::EPoint> proj(i1 - i0);
        std::vector<zkwit::JPoint> aff(i1 - i0);
        WipeOnExit wipe_p{proj.data(), proj.size() * sizeof(zkwit::EPoint)}, wipe_a{aff.data(), aff.size() * sizeof(zkwit::JPoint)};
        for (size_t i = i0; i < i1; i++) proj[i - i0] = zkwit::ext_add(jubjub_fixed_mul_ext(&c->f[4 * i]), parent);
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        for (size_t i = i0; i < i1; i++) {
            jubjub_encode(aff[i - i0].x, aff[i - i0].y, &c->pgk[32 * i]);
            dec_key_of(&c->pgk[32 * i], &c->dk[4 * i]);
            if (want_enc) proj[i - i0] = jubjub_fixed_mul_ext(&c->dk[4 * i]);
        }
        if (!want_enc) return ZK_OK;
        zkwit::batch_to_affine(proj.data(), aff.data(), proj.size());
        for (size_t i = i0; i < i1; i++) jubjub_encode(aff[i - i0].x, aff[i - i0].y, &c->enc[32 * i]);
        return ZK_OK;
    });
}
inline zk_status points_device(const Parent& p, size_t n, int device, Children* c) {
    ZK_TRY(zkrt::use_device(device));
    const uint32_t* tab = nullptr;
    ZK_TRY(device_table(device, &tab));
    const bool staged = stage_table();
    uint32_t parent[ENTRY_WORDS];
    {
        const zkhost::Fr e[3] = {p.pgk.y + p.pgk.x, p.pgk.y - p.pgk.x, p.pgk.x * p.pgk.y * zkwit::edwards_d().dbl()};
        memcpy(parent, e, 96);
    }
    zkrt::DevBuf in, out;   // f | dk among the output: zeroed before they go back, on every way out of this function
    std::vector<uint32_t> back(std::min(SLICE, n) * 24);
    WipeOnExit wipe_back{back.data(), back.size() * 4};
    for (size_t first = 0; first < n; first += SLICE) {
        const size_t np = std::min(SLICE, n - first);
        ZK_TRY(in.ensure(96 + np * 32));
        ZK_TRY(out.ensure(np * 96));
        {
            zkrt::ProfScope ps("hd_upload");
            HIP_TRY(hipMemcpyAsync(in.p, parent, 96, hipMemcpyHostToDevice, zkrt::g_stream));
            HIP_TRY(hipMemcpyAsync(in.as<uint8_t>() + 96, &c->f[4 * first], np * 32, hipMemcpyHostToDevice, zkrt::g_stream));
        }
        {
            zkrt::ProfScope ps("hd_children");
            launch_form(staged, k_hd_children<false>, k_hd_children<true>, np, tab, in.as<const uint32_t>(), in.as<const uint32_t>() + ENTRY_WORDS,
                        out.as<uint32_t>(), (uint32_t)np);
        }
        HIP_TRY(hipGetLastError());
        {
            zkrt::ProfScope ps("hd_download");
            HIP_TRY(hipMemcpyAsync(back.data(), out.p, np * 96, hipMemcpyDeviceToHost, zkrt::g_stream));
        }
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        for (size_t i = 0; i < np; i++) {
            memcpy(&c->pgk[32 * (first + i)], &back[24 * i], 32);
            memcpy(&c->dk[4 * (first + i)], &back[24 * i + 8], 32);
            memcpy(&c->enc[32 * (first + i)], &back[24 * i + 16], 32);
        }
    }
    return ZK_OK;
}
// the children of `xkey`: hashes, and the point work where the caller's outputs need it (need_points; want_enc: also [dk]G)
inline zk_status children(uint32_t kind, const uint8_t* xkey, const uint32_t* indices, size_t n, int device, bool need_points, bool want_enc,
                          Parent* p, Children* c) {
    ZK_TRY(parent_read(kind, xkey, p));
    ZK_TRY(check_indices(kind, *p, indices, n));
    ZK_TRY(hash_children(kind, *p, indices, n, c));
    if (!need_points) return ZK_OK;
    c->pgk.resize(n * 32);
    c->dk.resize(n * 4);
    c->enc.resize(n * 32);
    return device < 0 || n <= host_max() ? points_host(*p, n, want_enc, c) : points_device(*p, n, device, c);
}

inline zk_status master(const uint8_t* seed, size_t len, uint8_t* xsk_out) {
    zkhash::Blake2b h(MASTER_PERSON);
    uint8_t d[64];
    uint64_t sk[4];
    WipeOnExit wipe_h{&h, sizeof(h)}, wipe_d{d, sizeof(d)}, wipe_sk{sk, sizeof(sk)};
    h.update(seed, len);
    h.finish(d);
    expand_to_fs(d, 32, nullptr, 0, sk);   // SpendingKey::from_seed(I_L)
    const uint8_t tag[4] = {0, 0, 0, 0};
    xkey_write(xsk_out, 0, tag, 0, d + 32, reinterpret_cast<const uint8_t*>(sk));
    return ZK_OK;
}
inline zk_status xpgk_from_xsk(const uint8_t* xsk, uint8_t* xpgk_out) {
    Parent p;
    ZK_TRY(parent_read(ZK_HD_XSK, xsk, &p));
    uint8_t head[OFF_KEY];
    memcpy(head, xsk, OFF_KEY);   // (xpgk_out may be xsk)
    memcpy(xpgk_out, head, OFF_KEY);
    memcpy(xpgk_out + OFF_KEY, p.pgk_bytes, 32);
    return ZK_OK;
}
inline zk_status derive(uint32_t kind, const uint8_t* xkey, const uint32_t* indices, size_t n, int device, uint8_t* xkeys_out, uint8_t* dec_keys_out,
                        uint8_t* enc_keys_out) {
    ZK_TRY(check_kind(kind));
    if (n == 0) return ZK_OK;
    if (!xkey || !indices) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    Parent p;
    Children c;
    const bool need_points = dec_keys_out || enc_keys_out || (xkeys_out && kind == ZK_HD_XPGK);
    ZK_TRY(children(kind, xkey, indices, n, device, need_points, enc_keys_out != nullptr, &p, &c));
    // nothing was written so far, and nothing below fails
    for (size_t i = 0; xkeys_out && i < n; i++)
        xkey_write(xkeys_out + XKEY_BYTES * i, p.depth + 1u, p.tag, indices[i], &c.chain[32 * i],
                   kind == ZK_HD_XSK ? reinterpret_cast<const uint8_t*>(&c.sk[4 * i]) : &c.pgk[32 * i]);
    if (dec_keys_out) memcpy(dec_keys_out, c.dk.data(), n * 32);
    if (enc_keys_out) memcpy(enc_keys_out, c.enc.data(), n * 32);
    return ZK_OK;
}
// zk_scan_keys_create of the children's decryption keys, their encryption keys taken from the derivation
inline zk_status scan_keys_create(uint32_t kind, const uint8_t* xkey, const uint32_t* indices, size_t n, int device, zk_scan_keys** out) {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    ZK_TRY(check_kind(kind));
    if (!xkey || (n && !indices)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0 || n > 0xffffffffull) return fail(ZK_ERR_INVALID_ARGUMENT, "n_keys must be 1 .. 2^32 - 1");
    Parent p;
    Children c;
    ZK_TRY(children(kind, xkey, indices, n, device, true, true, &p, &c));
    std::unique_ptr<zk_scan_keys> k;
    ZK_TRY(zkscan::keys_load(reinterpret_cast<const uint8_t*>(c.dk.data()), n, &k));
    memcpy(k->enc.data(), c.enc.data(), n * 32);
    return zkscan::keys_index(std::move(k), out);
}

// n x [scalar_i] G (+ addend_i), always on the device
inline zk_status base_mul_dev(const uint8_t* scalars, const uint8_t* addends, size_t n, int device, uint8_t* points_out, uint8_t* status_out) {
    if (n == 0) return ZK_OK;
    if (!scalars || !points_out || (addends && !status_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; i++) {
        uint64_t k[4];
        WipeOnExit wipe_k{k, sizeof(k)};
        zkrt::load_scalar_le(scalars + 32 * i, k);
        if (!fs_lt_mod(k)) return fail(ZK_ERR_INVALID_ARGUMENT, "scalar " + std::to_string(i) + " is not a canonical Fs scalar");
    }
    ZK_TRY(zkrt::use_device(device));
    const uint32_t* tab = nullptr;
    ZK_TRY(device_table(device, &tab));
    const bool staged = stage_table();
    zkrt::DevBuf in, out;   // the scalars and their multiples may be a caller's secrets: zeroed before they go back
    std::vector<uint32_t> back(std::min(SLICE, n) * 9);
    WipeOnExit wipe_back{back.data(), back.size() * 4};
    for (size_t first = 0; first < n; first += SLICE) {
        const size_t np = std::min(SLICE, n - first), per_lane = addends ? 64 : 32;
        ZK_TRY(in.ensure(np * per_lane));
        ZK_TRY(out.ensure(np * 36));
        HIP_TRY(hipMemcpyAsync(in.p, scalars + 32 * first, np * 32, hipMemcpyHostToDevice, zkrt::g_stream));
        if (addends) HIP_TRY(hipMemcpyAsync(in.as<uint8_t>() + np * 32, addends + 32 * first, np * 32, hipMemcpyHostToDevice, zkrt::g_stream));
        const uint32_t *d_scalars = in.as<const uint32_t>(), *d_addends = addends ? d_scalars + np * 8 : nullptr;
        uint32_t *d_points = out.as<uint32_t>(), *d_status = d_points + np * 8;
        {
            zkrt::ProfScope ps("base_mul");
            launch_form(staged, k_base_mul<false>, k_base_mul<true>, np, tab, d_scalars, d_addends, d_points, d_status, (uint32_t)np);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(back.data(), out.p, np * (addends ? 36 : 32), hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(points_out + 32 * first, back.data(), np * 32);
        for (size_t i = 0; addends && i < np; i++) status_out[first + i] = (uint8_t)back[np * 8 + i];
    }
    return ZK_OK;
}

}  // namespace zkhd
