// libzkamd, verification half: PreparedVerifyingKey handles and batch verification (include/zkamd.h,
// "Verification").  Replaces, behind the C ABI:
//   prepare_verifying_key            core/bellman-verifier/src/verifier.rs:15-30
//   verify_proof                     core/bellman-verifier/src/verifier.rs:32-63   (call sites: the wallet's
//                                    check_proof core/proofs/src/confidential.rs:208-278, the runtime's
//                                    modules/zk-system/src/lib.rs:57-108)
//   PreparedVerifyingKey::read/write core/bellman-verifier/src/lib.rs:175-236 (zface/params/conf_vk.dat)
//   Proof::read                      core/bellman-verifier/src/lib.rs:67-110 (compressed points, into_affine)
//   verify_confidential_proof / verify_anonymous_proof   modules/zk-system/src/lib.rs:56-165 (the public inputs from the
//                                    extrinsic's bytes: PublicInputBuilder::push, IntoXY - xt_inputs.h)
//   rollover / sub_enc_balance / add_pending_transfer    modules/encrypted-balances/src/lib.rs:133-222, encrypted-assets :266-350,
//                                    anonymous-balances :169-225 (a block's Ciphertext::add / sub in order - ledger.h)
// Device side: pairing.h.  Host side here: byte formats, the handle, the launch sequence.
#include <algorithm>
#include <new>

#include "host_common.h"
#include "host_math.h"
#include "blake2s.h"
#include "pairing.h"
#include "msm_point_kernels.h"   // (k_import_affine / k_check_points over the saturated Fq2: this unit is their one user)
#include "msm_group.h"           // (check_points_host, import_affine_dev, build_table_dev over G1: msm_g1.cpp)
#include "coop_verify.h"
#include "xt_inputs.h"
#include "ledger.h"
#include "block_exec.h"
#include "anon_block_exec.h"
#include "asset_block_exec.h"
#include "verify_plan.h"
#include "verify_rlc.h"

using namespace zkrt;
using zkdev::F12;

namespace {

typedef zkhost::Affine<zkhost::Fq> HG1A;
typedef zkhost::Affine<zkhost::Fq2> HG2A;
typedef zkdev::Affine<zkdev::Fq> DG1A;    // radix-2^28 form (tables of the input accumulator)
typedef zkdev::XYZZ<zkdev::Fq> DG1;

struct Reader {
    const uint8_t* p;
    size_t left;
    bool take(size_t n, const uint8_t** out) {
        if (left < n) return false;
        *out = p;
        p += n;
        left -= n;
        return true;
    }
    bool u32be(uint32_t* v) {
        const uint8_t* b;
        if (!take(4, &b)) return false;
        *v = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        return true;
    }
};
void put_u32be(std::vector<uint8_t>& o, uint32_t v) {
    o.push_back((uint8_t)(v >> 24));
    o.push_back((uint8_t)(v >> 16));
    o.push_back((uint8_t)(v >> 8));
    o.push_back((uint8_t)v);
}

// 48 big-endian bytes (top `mask` bits cleared) -> 12 plain little-endian u32 words; false if >= q
bool fq_words_from_be(const uint8_t* b, uint32_t* w, uint8_t top_mask) {
    uint64_t l[6];
    for (int i = 0; i < 6; i++) {
        uint64_t v = 0;
        for (int j = 0; j < 8; j++) {
            uint8_t byte = b[(5 - i) * 8 + j];
            if (i == 5 && j == 0) byte &= top_mask;
            v = (v << 8) | byte;
        }
        l[i] = v;
    }
    if (zkhost::Fq::geq_p(l)) return false;
    for (int i = 0; i < 6; i++) {
        w[2 * i] = (uint32_t)l[i];
        w[2 * i + 1] = (uint32_t)(l[i] >> 32);
    }
    return true;
}
// Fq2::read / write (fq2.rs:40-60): c0 then c1, 48 big-endian bytes each, canonical
bool fq2_read(Reader& r, zkhost::Fq2* out) {
    const uint8_t* b;
    if (!r.take(96, &b)) return false;
    return zkhost::fq_from_be(b, &out->c0) && zkhost::fq_from_be(b + 48, &out->c1);
}
void fq2_write(std::vector<uint8_t>& o, const zkhost::Fq2& v) {
    uint8_t b[96];
    zkhost::fq_to_be(v.c0, b);
    zkhost::fq_to_be(v.c1, b + 48);
    o.insert(o.end(), b, b + 96);
}
zkhost::Fq2 fq2_pow(const zkhost::Fq2& a, const uint64_t* e, int n) {
    zkhost::Fq2 r = zkhost::Fq2::one();
    for (int i = n - 1; i >= 0; i--)
        for (int b = 63; b >= 0; b--) {
            r = r.sqr();
            if ((e[i] >> b) & 1) r = r * a;
        }
    return r;
}

zk_status read_g1(Reader& r, HG1A* out, const char* what, bool allow_inf) {
    const uint8_t* b;
    if (!r.take(96, &b)) return fail(ZK_ERR_IO, std::string("unexpected end of the key in ") + what);
    if (zkhost::g1_from_uncompressed(b, out) != zkhost::DEC_OK) return fail(ZK_ERR_IO, std::string("invalid G1 encoding in ") + what);
    if (!allow_inf && out->is_inf()) return fail(ZK_ERR_IO, std::string("point at infinity in ") + what);
    return ZK_OK;
}
zk_status read_g2(Reader& r, HG2A* out, const char* what) {
    const uint8_t* b;
    if (!r.take(192, &b)) return fail(ZK_ERR_IO, std::string("unexpected end of the key in ") + what);
    if (zkhost::g2_from_uncompressed(b, out) != zkhost::DEC_OK) return fail(ZK_ERR_IO, std::string("invalid G2 encoding in ") + what);
    return ZK_OK;
}

constexpr size_t COEF_WORDS = (size_t)zkdev::PAIRING_NCOEF * 72;
constexpr size_t VERIFY_CHUNK = 8192;   // proofs per launch set

// The lane's three streams around a chunk: main forks into (side, copy), each says when it is done, main waits for both
struct ForkJoin {
    hipEvent_t done[2] = {nullptr, nullptr};   // side, copy: created on first use
    ~ForkJoin() {
        for (int k = 0; k < 2; k++)
            if (done[k]) (void)hipEventDestroy(done[k]);
    }
    zk_status fork() {
        for (int k = 0; k < 2; k++)
            if (!done[k]) HIP_TRY(hipEventCreate(&done[k]));
        HIP_TRY(hipEventRecord(g_ev_fork, g_stream));
        HIP_TRY(hipStreamWaitEvent(g_stream2, g_ev_fork, 0));
        HIP_TRY(hipStreamWaitEvent(g_copy_stream, g_ev_fork, 0));
        return ZK_OK;
    }
    zk_status side_done() {
        HIP_TRY(hipEventRecord(done[0], g_stream2));
        return ZK_OK;
    }
    zk_status copy_done() {
        HIP_TRY(hipEventRecord(done[1], g_copy_stream));
        return ZK_OK;
    }
    zk_status join() {
        HIP_TRY(hipStreamWaitEvent(g_stream, done[0], 0));
        HIP_TRY(hipStreamWaitEvent(g_stream, done[1], 0));
        return ZK_OK;
    }
};

// The workspaces of the random-linear-combination check alone (verify_chunk_rlc; skip, f, ok and prep_b it shares with the
// per-proof path)
struct RlcWork {
    typedef zkdev::XYZZ<zkdev::Fq32> P32;
    DevBuf rho, s, exp;     // the coefficients of the chunk (verify_rlc.h Coefs)
    DevBuf pts;             // rho_i A_i | acc | C sum: the G1 side of the n + 2 pairs
    DevBuf c, csum;         // rho_i C_i, and their sum in front of its partial sums of 256
    DevBuf acc, inf, all;   // sum_j s_j ic_j; is acc / the C sum the point at infinity; is every proof well-formed
    DevBuf want, prod;      // e(alpha, beta)^S; the two halves of the product tree's workspace
    DevBuf fe, ab_lambda;   // once per key (ensure_rlc_fe, ensure_rlc_ab_lambda)
    zk_status reserve(size_t n, uint32_t n_ic) {
        const size_t m = n + 2;
        ZK_TRY(rho.ensure(n * 16));
        ZK_TRY(s.ensure((size_t)n_ic * 32));
        ZK_TRY(exp.ensure(32));
        ZK_TRY(pts.ensure(m * 96));
        ZK_TRY(c.ensure(n * sizeof(P32)));
        ZK_TRY(csum.ensure(((n + 255) / 256 + 1) * sizeof(P32)));
        ZK_TRY(acc.ensure(sizeof(DG1)));
        ZK_TRY(inf.ensure(8));
        ZK_TRY(all.ensure(4));
        ZK_TRY(want.ensure(sizeof(F12)));
        ZK_TRY(prod.ensure(2 * prod_half(m) * sizeof(F12)));
        return ZK_OK;
    }
    static size_t prod_half(size_t m) { return m / 12 + 2; }   // (the first level of m functions leaves (m + 11) / 12 products)
};

}  // namespace

struct zk_vk {
    int device = 0;
    uint32_t n_ic = 0;
    bool gamma_inf = false, delta_inf = false;
    std::vector<HG1A> ic;
    std::vector<uint32_t> h_alpha_beta;          // 144 words: the Fq12 in tower order, Montgomery
    std::vector<uint32_t> h_prep[2];             // 68 x 72 words each (-gamma, -delta); empty = infinity
    DevBuf ic_table, prep[2], gam, alpha_beta;
    // per-batch workspaces
    DevBuf in_g1, in_g2, fl_g1, fl_g2, aff_g1, aff_g2, st_g1, st_g2, scal, part, acc, acc_inf, host_bad, skip, valid, f, ok;
    DevBuf coop_stage;   // the cooperative line preparation's un-reduced coefficients (coop_verify.cpp)
    DevBuf ic_win;       // the 8-bit window table of the ic bases (pairing.h k_inputs_window_table): ensure_ic_win
    DevBuf lines28[2];   // prep[] in the multiexps' representation, for the Miller loop on rows (coop_pairing.cpp): ensure_lines28
    DevBuf prep_b;   // line coefficients of the batch's own B points (the lane-parallel Miller loop reads every pair prepared)
    RlcWork rlc;
    zkxt::IntoXyBufs xt;    // IntoXY of the extrinsics' points (xt_inputs.h)
    DevBuf block;           // the block executor's ledger layout, scan results and public inputs (block_exec.h; public chain state)
    PinBuf block_rows;      // ... and the rows of public inputs of a round on their way into verify_batch
    // the G1 decoder and the input accumulator run beside the G2 decoder on the lane's side streams
    ForkJoin streams;
    // Blake2s over e(alpha, beta), the prepared -gamma / -delta coefficients and ic: the domain separation of the combined
    // check's coefficients (the same batch bytes under another key draw other rho_i)
    uint8_t key_digest[32] = {0};
};

namespace {

zk_status upload(DevBuf& d, const void* src, size_t bytes) {
    ZK_TRY(d.ensure(bytes ? bytes : 4));
    if (bytes) HIP_TRY(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, g_stream));
    return ZK_OK;
}

// xi^(i (q^k - 1) / 6) for k = 1, 2 and i = 0 .. 5  (pairing.h f12_frob)
zk_status upload_frobenius(zk_vk* V) {
    static const uint64_t e[6] = ZK_FQ_EXP_QM1D6_64;
    const zkhost::Fq2 xi{zkhost::Fq::one(), zkhost::Fq::one()};
    const zkhost::Fq2 g = fq2_pow(xi, e, 6);
    std::vector<zkhost::Fq2> tab(12);
    zkhost::Fq2 p = zkhost::Fq2::one();
    for (int i = 0; i < 6; i++) {
        tab[i] = p;
        const zkhost::Fq2 conj{p.c0, -p.c1};
        tab[6 + i] = p * conj;
        p = p * g;
    }
    static_assert(sizeof(zkhost::Fq2) == 96, "Fq2 layout");
    ZK_TRY(upload(V->gam, tab.data(), tab.size() * sizeof(zkhost::Fq2)));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
}

// on-curve and subgroup validation of decoded key points (into_affine): the prover's kernel.  G1 points go through the
// prover's own function (check_points_host, msm_g1.cpp); the G2 points of a key live on the saturated Fq2 here.
zk_status check_points_g2(const std::vector<HG2A>& pts, const char* what) {
    typedef zkdev::Fq2 DF;
    if (pts.empty()) return ZK_OK;
    const size_t n = pts.size();
    DevBuf stage, d, flags;
    ZK_TRY(upload(stage, pts.data(), n * sizeof(HG2A)));
    ZK_TRY(d.ensure(n * sizeof(zkdev::Affine<DF>)));
    ZK_TRY(flags.ensure(4 * n));
    const unsigned blocks = (unsigned)((n + 127) / 128);
    ZK_LAUNCH(zkdev::k_import_affine<DF>, dim3(blocks), dim3(128), 0, g_stream, stage.as<const uint32_t>(),
              d.as<zkdev::Affine<DF>>(), (uint32_t)n);
    ZK_LAUNCH(zkdev::k_check_points<DF>, dim3(blocks), dim3(128), 0, g_stream, d.as<const zkdev::Affine<DF>>(),
              (uint32_t)n, 1u, flags.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> f(n);
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(f.data(), flags.p, 4 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        if (f[i])
            return fail(ZK_ERR_IO, std::string(what) + ": point " + std::to_string(i) +
                                       (f[i] & 1 ? " is not on the curve" : " is not in the correct subgroup"));
    return ZK_OK;
}

// the doubling table of the ic bases: table[k][j] = 2^k ic[j]
zk_status build_ic_table(zk_vk* V) {
    const size_t n = V->ic.size();
    V->n_ic = (uint32_t)n;
    if (!n) return ZK_OK;
    ZK_TRY(V->ic_table.ensure(sizeof(DG1A) * n * zkdev::MSM_NPOS));
    DevBuf stage, scratch;
    ZK_TRY(upload(stage, V->ic.data(), n * sizeof(HG1A)));
    ZK_TRY(import_affine_dev<zkdev::Fq>(stage.p, V->ic_table.as<DG1A>(), n, g_stream));
    ZK_TRY(build_table_dev<zkdev::Fq>(V->ic_table.as<DG1A>(), n, zkdev::MSM_NPOS, scratch, 1u, 0u, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return ZK_OK;
}

struct VkGuard {   // a key under construction: freed on every way out but the last
    zk_vk* p;
    ~VkGuard() { delete p; }
};
zk_status vk_prepare(const uint8_t* bytes, size_t len, int device, zk_vk** out) {
    ZK_TRY(use_device(device));
    zk_vk* V = new (std::nothrow) zk_vk();
    if (!V) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    VkGuard guard{V};
    V->device = device;
    Reader r{bytes, len};
    HG1A alpha_g1, beta_g1, delta_g1, tmp;
    HG2A beta_g2, gamma_g2, delta_g2;
    // VerifyingKey::read (in-tree twin: core/bellman-verifier/src/lib.rs:305-355): infinity is accepted for the
    // six named points, rejected inside ic
    ZK_TRY(read_g1(r, &alpha_g1, "vk.alpha_g1", true));
    ZK_TRY(read_g1(r, &beta_g1, "vk.beta_g1", true));
    ZK_TRY(read_g2(r, &beta_g2, "vk.beta_g2"));
    ZK_TRY(read_g2(r, &gamma_g2, "vk.gamma_g2"));
    ZK_TRY(read_g1(r, &delta_g1, "vk.delta_g1", true));
    ZK_TRY(read_g2(r, &delta_g2, "vk.delta_g2"));
    uint32_t n_ic = 0;
    if (!r.u32be(&n_ic)) return fail(ZK_ERR_IO, "unexpected end of the key (ic length)");
    if ((size_t)n_ic * 96 > r.left) return fail(ZK_ERR_IO, "unexpected end of the key in vk.ic");
    for (uint32_t i = 0; i < n_ic; i++) {
        ZK_TRY(read_g1(r, &tmp, "vk.ic", false));
        V->ic.push_back(tmp);
    }
    {
        std::vector<HG1A> g1 = V->ic;
        g1.push_back(alpha_g1);
        g1.push_back(beta_g1);
        g1.push_back(delta_g1);
        ZK_TRY((check_points_host<zkhost::Fq, zkdev::Fq>(g1, "vk (G1: ic | alpha | beta | delta)")));
        ZK_TRY(check_points_g2(std::vector<HG2A>{beta_g2, gamma_g2, delta_g2}, "vk (G2: beta | gamma | delta)"));
    }
    ZK_TRY(upload_frobenius(V));
    ZK_TRY(build_ic_table(V));
    // neg_gamma_g2, neg_delta_g2 prepared on the GPU
    V->gamma_inf = gamma_g2.is_inf();
    V->delta_inf = delta_g2.is_inf();
    const HG2A neg[2] = {HG2A{gamma_g2.x, -gamma_g2.y}, HG2A{delta_g2.x, -delta_g2.y}};
    {
        DevBuf q, co;
        ZK_TRY(upload(q, neg, sizeof(neg)));
        ZK_TRY(co.ensure(2 * COEF_WORDS * 4));
        ZK_LAUNCH(zkdev::k_g2_prepare, dim3(1), dim3(64), 0, g_stream, q.as<const uint32_t>(), co.as<uint32_t>(), 2u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g_stream));
        for (int k = 0; k < 2; k++) {
            if (k == 0 ? V->gamma_inf : V->delta_inf) continue;
            V->h_prep[k].resize(COEF_WORDS);
            HIP_TRY(hipMemcpy(V->h_prep[k].data(), co.as<uint32_t>() + k * COEF_WORDS, COEF_WORDS * 4, hipMemcpyDeviceToHost));
            ZK_TRY(upload(V->prep[k], V->h_prep[k].data(), COEF_WORDS * 4));
        }
    }
    // alpha_g1_beta_g2 = e(alpha, beta)
    {
        DevBuf p0, q0, sk, f, val;
        uint32_t skip = (alpha_g1.is_inf() || beta_g2.is_inf()) ? 1u : 0u;
        ZK_TRY(upload(p0, &alpha_g1, sizeof(alpha_g1)));
        ZK_TRY(upload(q0, &beta_g2, sizeof(beta_g2)));
        ZK_TRY(upload(sk, &skip, 4));
        ZK_TRY(f.ensure(3 * sizeof(F12)));
        ZK_TRY(val.ensure(sizeof(F12)));
        ZK_LAUNCH(zkdev::k_miller_loop, dim3(1, 3), dim3(64), 0, g_stream, p0.as<const uint32_t>(),
                  q0.as<const uint32_t>(), (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                  (const uint32_t*)nullptr, sk.as<const uint32_t>(), f.as<F12>(), 1u);
        ZK_LAUNCH(zkdev::k_final_exp, dim3(1), dim3(64), 0, g_stream, f.as<const F12>(), V->gam.as<const uint32_t>(),
                  (const F12*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, val.as<F12>(), 1u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g_stream));
        static_assert(sizeof(F12) == 144 * 4, "Fq12 layout");
        V->h_alpha_beta.resize(144);
        HIP_TRY(hipMemcpy(V->h_alpha_beta.data(), val.p, sizeof(F12), hipMemcpyDeviceToHost));
        ZK_TRY(upload(V->alpha_beta, V->h_alpha_beta.data(), sizeof(F12)));
    }
    HIP_TRY(hipStreamSynchronize(g_stream));
    guard.p = nullptr;
    *out = V;
    return ZK_OK;
}

void vk_digest(zk_vk* V) {
    static const uint8_t pers[8] = {'z', 'k', 'a', 'm', 'd', 'v', 'k', 'd'};
    zkhash::Blake2s h(pers);
    h.update(V->h_alpha_beta.data(), V->h_alpha_beta.size() * 4);
    for (int k = 0; k < 2; k++) {
        h.update_u64be(V->h_prep[k].size());
        h.update(V->h_prep[k].data(), V->h_prep[k].size() * 4);
    }
    h.update_u64be(V->ic.size());
    for (const HG1A& p : V->ic) {
        uint8_t b[96];
        zkhost::g1_to_uncompressed(p, b);
        h.update(b, 96);
    }
    h.finish(V->key_digest);
}

// PreparedVerifyingKey::read (core/bellman-verifier/src/lib.rs:207-244)
zk_status vk_read_prepared(const uint8_t* bytes, size_t len, int device, zk_vk** out) {
    ZK_TRY(use_device(device));
    zk_vk* V = new (std::nothrow) zk_vk();
    if (!V) return fail(ZK_ERR_OUT_OF_MEMORY, "host allocation failed");
    VkGuard guard{V};
    V->device = device;
    Reader r{bytes, len};
    zkhost::Fq2 c;
    static_assert(sizeof(zkhost::Fq2) == 24 * 4, "Fq2 layout");
    V->h_alpha_beta.resize(144);
    for (int i = 0; i < 6; i++) {   // Fq12::read: c0 (c0, c1, c2), c1 (c0, c1, c2)
        if (!fq2_read(r, &c)) return fail(ZK_ERR_IO, "alpha_g1_beta_g2: short or not in the field");
        memcpy(&V->h_alpha_beta[i * 24], &c, 96);
    }
    for (int k = 0; k < 2; k++) {   // G2Prepared::read (ec.rs:1655-1683)
        const char* what = k == 0 ? "neg_gamma_g2" : "neg_delta_g2";
        uint32_t cnt = 0;
        if (!r.u32be(&cnt)) return fail(ZK_ERR_IO, std::string(what) + ": unexpected end");
        if ((size_t)cnt * 288 > r.left) return fail(ZK_ERR_IO, std::string(what) + ": unexpected end");
        std::vector<uint32_t> co((size_t)cnt * 72);
        for (uint32_t i = 0; i < cnt * 3; i++) {
            if (!fq2_read(r, &c)) return fail(ZK_ERR_IO, std::string(what) + ": coefficient not in the field");
            memcpy(&co[(size_t)i * 24], &c, 96);
        }
        const uint8_t* flag;
        if (!r.take(1, &flag) || *flag > 1) return fail(ZK_ERR_IO, std::string(what) + ": bad infinity flag");
        const bool inf = *flag == 1;
        if (!inf && cnt != (uint32_t)zkdev::PAIRING_NCOEF)
            return fail(ZK_ERR_IO, std::string(what) + ": expected " + std::to_string(zkdev::PAIRING_NCOEF) + " coefficient triples");
        (k == 0 ? V->gamma_inf : V->delta_inf) = inf;
        if (!inf) {
            V->h_prep[k] = co;
            ZK_TRY(upload(V->prep[k], V->h_prep[k].data(), COEF_WORDS * 4));
        }
    }
    uint32_t n_ic = 0;
    if (!r.u32be(&n_ic)) return fail(ZK_ERR_IO, "unexpected end of the key (ic length)");
    if ((size_t)n_ic * 96 > r.left) return fail(ZK_ERR_IO, "unexpected end of the key in ic");
    HG1A tmp;
    for (uint32_t i = 0; i < n_ic; i++) {
        ZK_TRY(read_g1(r, &tmp, "ic", false));
        V->ic.push_back(tmp);
    }
    ZK_TRY((check_points_host<zkhost::Fq, zkdev::Fq>(V->ic, "ic")));
    ZK_TRY(upload(V->alpha_beta, V->h_alpha_beta.data(), 144 * 4));
    ZK_TRY(upload_frobenius(V));
    ZK_TRY(build_ic_table(V));
    HIP_TRY(hipStreamSynchronize(g_stream));
    vk_digest(V);
    guard.p = nullptr;
    *out = V;
    return ZK_OK;
}

// one element of a Proof: compressed encoding of `len` bytes (48: G1, 96: G2) -> plain x words + flags (bit 0 infinity, bit 1
// larger y); false = malformed (Proof::read fails: ec.rs:776-868, :1429-1548)
bool parse_compressed(const uint8_t* b, size_t len, uint32_t* x, uint32_t* flags) {
    if (!(b[0] & 0x80)) return false;   // not the compressed form
    if (b[0] & 0x40) {
        if ((b[0] & 0x3f) || std::any_of(b + 1, b + len, [](uint8_t v) { return v != 0; })) return false;
        *flags = 1;
        memset(x, 0, len);
        return true;
    }
    *flags = (b[0] & 0x20) ? 2u : 0u;
    if (len == 48) return fq_words_from_be(b, x, 0x1f);
    return fq_words_from_be(b, x + 12, 0x1f) && fq_words_from_be(b + 48, x, 0xff);   // c1 first on the wire
}
bool parse_g1_compressed(const uint8_t* b, uint32_t* x, uint32_t* flags) { return parse_compressed(b, 48, x, flags); }
bool parse_g2_compressed(const uint8_t* b, uint32_t* x, uint32_t* flags) { return parse_compressed(b, 96, x, flags); }

// The front end of a chunk (verify_chunk, verify_chunk_rlc, zk_proof_read_batch), what the host makes of n proofs:
// x words and flag words of A | C (g1, f1: C behind the n A's) and of B (g2, f2); enc[i] bit k: the ENCODING of point k (0 = A,
// 1 = B, 2 = C) is refused, that point decodes to nothing
struct Staged {
    std::vector<uint32_t> g1, g2, f1, f2;
    std::vector<uint8_t> enc;
    // every point is parsed on its own: Proof::read finishes A (decode, curve, subgroup, infinity) before it touches B, so a
    // device-side failure of A must win over a malformed B.  proofs == nullptr: nothing to parse, all zero
    Staged(size_t n, const uint8_t* proofs) : g1((size_t)2 * n * 12), g2((size_t)n * 24), f1(2 * n), f2(n), enc(n, 0) {
        for (size_t i = 0; proofs && i < n; i++) {
            const uint8_t* p = proofs + i * 192;
            auto refused = [&](int k, uint32_t* x, size_t words, uint32_t* flag) {
                enc[i] |= (uint8_t)(1u << k);
                *flag = 1;   // decode nothing
                memset(x, 0, words * 4);
            };
            if (!parse_g1_compressed(p, &g1[i * 12], &f1[i])) refused(0, &g1[i * 12], 12, &f1[i]);
            if (!parse_g2_compressed(p + 48, &g2[i * 24], &f2[i])) refused(1, &g2[i * 24], 24, &f2[i]);
            if (!parse_g1_compressed(p + 144, &g1[(n + i) * 12], &f1[n + i])) refused(2, &g1[(n + i) * 12], 12, &f1[n + i]);
        }
    }
};
// ni public inputs of one proof, 32 little-endian bytes each: all canonical Fr?  (Of another the reference cannot even form the input.)
bool inputs_canonical(const uint8_t* row, uint32_t ni) {
    for (uint32_t j = 0; j < ni; j++) {
        uint64_t v[4];
        load_scalar_le(row + j * 32, v);
        if (zkhost::Fr::geq_p(v)) return false;
    }
    return true;
}
// the staged words uploaded, the decoders' outputs reserved; bad: the host's verdict per proof, of the callers that have one
zk_status upload_staged(zk_vk* V, size_t n, const Staged& s, const std::vector<uint32_t>* bad) {
    ZK_TRY(upload(V->in_g1, s.g1.data(), s.g1.size() * 4));
    ZK_TRY(upload(V->in_g2, s.g2.data(), s.g2.size() * 4));
    ZK_TRY(upload(V->fl_g1, s.f1.data(), s.f1.size() * 4));
    ZK_TRY(upload(V->fl_g2, s.f2.data(), s.f2.size() * 4));
    if (bad) ZK_TRY(upload(V->host_bad, bad->data(), bad->size() * 4));
    ZK_TRY(V->aff_g1.ensure((size_t)2 * n * 96));
    ZK_TRY(V->aff_g2.ensure(n * 192));
    ZK_TRY(V->st_g1.ensure(2 * n * 4));
    ZK_TRY(V->st_g2.ensure(n * 4));
    return ZK_OK;
}
// B decoded and its lines prepared on `main`, A | C decoded on `side`, in the forms the plan names
zk_status enqueue_head(zk_vk* V, size_t n, const VerifyPlan& pl, hipStream_t main, hipStream_t side) {
    const uint32_t *in_g1 = V->in_g1.as<const uint32_t>(), *in_g2 = V->in_g2.as<const uint32_t>();
    const uint32_t *fl_g1 = V->fl_g1.as<const uint32_t>(), *fl_g2 = V->fl_g2.as<const uint32_t>();
    uint32_t *aff_g1 = V->aff_g1.as<uint32_t>(), *aff_g2 = V->aff_g2.as<uint32_t>(), *st_g1 = V->st_g1.as<uint32_t>(), *st_g2 = V->st_g2.as<uint32_t>();
    {
        ProfScope ps("verify_decode", main);
        if (pl.decode == VDecode::ROWS)
            zkcoop::verify_decode_g2(in_g2, fl_g2, aff_g2, st_g2, (uint32_t)n, main);
        else if (pl.decode == VDecode::LANES)
            ZK_LAUNCH(zkdev::k_decode_g2, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, main, in_g2, fl_g2, aff_g2, st_g2, (uint32_t)n,
                      pl.b_torsion_in_decoder ? 1u : 0u);
    }
    static_assert(zkcoop::VERIFY_NCOEF == zkdev::PAIRING_NCOEF, "coop_verify.cpp restates the loop constants");
    if (pl.prepare != VPrepare::NONE) {
        uint32_t* st_b = pl.subgroup_tests ? st_g2 : nullptr;   // (it skips what did not decode and settles B's r-torsion test)
        if (pl.prep_b_points) ZK_TRY(V->prep_b.ensure(pl.prep_b_points * COEF_WORDS * 4));
        if (pl.prepare == VPrepare::ROWS) ZK_TRY(V->coop_stage.ensure(zkcoop::g2_prepare_stage_bytes((uint32_t)n)));
        ProfScope ps("verify_prepare", main);
        if (pl.prepare == VPrepare::ROWS)
            zkcoop::verify_g2_prepare(aff_g2, V->coop_stage.p, pl.prep_b_points ? V->prep_b.as<uint32_t>() : nullptr, (uint32_t)n, st_b, main);
        else
            ZK_LAUNCH_SYNC(zkdev::k_g2_prepare_tri, dim3((unsigned)((n + zkdev::TL_POINTS - 1) / zkdev::TL_POINTS)), dim3(64), 0, main,
                           (const uint32_t*)aff_g2, V->prep_b.as<uint32_t>(), (uint32_t)n, st_b);
    }
    {
        ProfScope ps("verify_decode_g1", side);
        const uint32_t check = pl.subgroup_tests ? 1u : 0u;
        if (pl.decode == VDecode::ROWS)
            zkcoop::verify_decode_g1(in_g1, fl_g1, aff_g1, st_g1, (uint32_t)(2 * n), check, side);
        else if (pl.decode == VDecode::LANES)
            ZK_LAUNCH(zkdev::k_decode_g1, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, side, in_g1, fl_g1, aff_g1, st_g1, (uint32_t)(2 * n), check);
    }
    return ZK_OK;
}
// the prover's affine A, B, C (host_common.h OWN_AFFINE_BYTES per proof) uploaded where the decoders would have left them:
// [A | C] and B, "decoded" in every state word
zk_status stage_own_affine(zk_vk* V, size_t n, const uint8_t* own_affine) {
    std::vector<uint8_t> a1((size_t)2 * n * 96), a2(n * 192);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* a = own_affine + i * OWN_AFFINE_BYTES;
        memcpy(&a1[i * 96], a, 96);
        memcpy(&a1[(n + i) * 96], a + 288, 96);
        memcpy(&a2[i * 192], a + 96, 192);
    }
    ZK_TRY(upload(V->in_g1, a1.data(), a1.size()));   // (staged through the buffers the encodings would have used)
    ZK_TRY(upload(V->in_g2, a2.data(), a2.size()));
    HIP_TRY(hipMemcpyAsync(V->aff_g1.p, V->in_g1.p, a1.size(), hipMemcpyDeviceToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(V->aff_g2.p, V->in_g2.p, a2.size(), hipMemcpyDeviceToDevice, g_stream));
    HIP_TRY(hipMemsetAsync(V->st_g1.p, 0, 2 * n * 4, g_stream));
    HIP_TRY(hipMemsetAsync(V->st_g2.p, 0, n * 4, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));   // (a1 / a2 are about to go out of scope: pageable sources of asynchronous copies)
    return ZK_OK;
}
// The four device tables of a key that are built on first use, once per key, each on the stream of the stage that reads it:
// the window table of the ic bases (public) ...
zk_status ensure_ic_win(zk_vk* V, hipStream_t st) {
    if (V->ic_win.cap) return ZK_OK;
    V->ic_win.is_public = true;
    ZK_TRY(V->ic_win.ensure((size_t)V->n_ic * 32 * 256 * sizeof(DG1A)));
    ZK_LAUNCH(zkdev::k_inputs_window_table, dim3((unsigned)(V->n_ic * 32 * 256 / 64)), dim3(64), 0, st, V->ic_table.as<const DG1A>(), V->ic_win.as<DG1A>(),
              V->n_ic);
    return ZK_OK;
}
// ... the key's prepared lines in the rows' representation (public) ...
zk_status ensure_lines28(zk_vk* V, hipStream_t st) {
    for (int k = 0; k < 2; k++) {
        if ((k == 0 ? V->gamma_inf : V->delta_inf) || V->lines28[k].cap) continue;
        V->lines28[k].is_public = true;
        ZK_TRY(V->lines28[k].ensure(zkcoop::LINE_TABLE_BYTES));
        zkcoop::verify_import_coefs(V->prep[k].as<const uint32_t>(), V->lines28[k].p, (uint32_t)zkcoop::VERIFY_NCOEF * 6, st);
    }
    return ZK_OK;
}
// ... [product | 1 | 1], what k_final_exp_wide multiplies for the one item of the combined check ...
zk_status ensure_rlc_fe(zk_vk* V, hipStream_t st) {
    if (V->rlc.fe.cap) return ZK_OK;
    static const std::vector<uint32_t> ones = [] {   // (static: the pageable source of an asynchronous copy)
        std::vector<uint32_t> o(3 * 144, 0);
        static const uint32_t R32[12] = ZK_FQ_R_32;
        for (int k = 1; k < 3; k++) memcpy(&o[(size_t)k * 144], R32, 48);
        return o;
    }();
    ZK_TRY(V->rlc.fe.ensure(ones.size() * 4));
    HIP_TRY(hipMemcpyAsync(V->rlc.fe.p, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, st));
    return ZK_OK;
}
// ... and e(alpha, beta)^lambda (the coefficients are a_i + b_i lambda: verify_rlc.h, pairing.h k_rlc_scale); the call that
// builds it waits for it
zk_status ensure_rlc_ab_lambda(zk_vk* V, hipStream_t st) {
    if (V->rlc.ab_lambda.cap) return ZK_OK;
    const zkhost::Fr lambda = zkrlc::lambda();
    DevBuf dl;
    ZK_TRY(dl.ensure(32));
    HIP_TRY(hipMemcpy(dl.p, lambda.l, 32, hipMemcpyHostToDevice));
    ZK_TRY(V->rlc.ab_lambda.ensure(sizeof(F12)));
    ZK_LAUNCH_SYNC(zkdev::k_f12_pow_wide, dim3(1), dim3(zkdev::W3_THREADS), 0, st, V->alpha_beta.as<const F12>(), dl.as<const uint32_t>(), 255u,
                   V->rlc.ab_lambda.as<F12>());
    HIP_TRY(hipStreamSynchronize(st));
    return ZK_OK;
}
// acc[p] = ic_0 + sum_j x_pj ic_j for the n proofs of the chunk, on `st`
zk_status enqueue_inputs(zk_vk* V, size_t n, const VerifyPlan& pl, hipStream_t st) {
    const uint32_t ni = V->n_ic - 1;
    const DG1A* table = V->ic_table.as<const DG1A>();
    const uint32_t* scal = V->scal.as<const uint32_t>();
    DG1* part = V->part.as<DG1>();
    uint32_t *acc = V->acc.as<uint32_t>(), *acc_inf = V->acc_inf.as<uint32_t>();
    ProfScope ps("verify_inputs", st);
    if (pl.inputs == VInputs::ROWS) {
        zkcoop::verify_inputs(V->ic_table.p, scal, V->part.p, acc, acc_inf, V->n_ic, (uint32_t)n, st);
        return ZK_OK;
    }
    // on lanes: the products of the pieces of every scalar with its base ...
    const bool sixteen = pl.inputs == VInputs::SIXTEEN;
    if (pl.inputs == VInputs::WINDOWS) {   // (four chains of eight additions per scalar)
        ZK_TRY(ensure_ic_win(V, st));
        ZK_LAUNCH(zkdev::k_inputs_mul_win<4>, dim3((unsigned)((4 * n * ni + 63) / 64)), dim3(64), 0, st, V->ic_win.as<const DG1A>(), scal, part,
                  V->n_ic, (uint32_t)n);
    } else if (pl.inputs_mul && sixteen) {
        ZK_LAUNCH(zkdev::k_inputs_mul<16>, dim3((unsigned)((16 * n * ni + 63) / 64)), dim3(64), 0, st, table, scal, part, V->n_ic, (uint32_t)n);
    } else if (pl.inputs_mul) {
        ZK_LAUNCH(zkdev::k_inputs_mul<4>, dim3((unsigned)((4 * n * ni + 63) / 64)), dim3(64), 0, st, table, scal, part, V->n_ic, (uint32_t)n);
    }
    if (sixteen)   // ... and their sum: a wave per proof
        ZK_LAUNCH_SYNC((zkdev::k_inputs_sum<16, 64>), dim3((unsigned)n), dim3(64), 0, st, table, (const DG1*)part, acc, acc_inf, V->n_ic, (uint32_t)n);
    else
        ZK_LAUNCH_SYNC((zkdev::k_inputs_sum<4, 8>), dim3((unsigned)((n + 7) / 8)), dim3(64), 0, st, table, (const DG1*)part, acc, acc_inf, V->n_ic,
                       (uint32_t)n);
    return ZK_OK;
}
// e(A, B) e(acc, -gamma) e(C, -delta) == e(alpha, beta) per proof: three Miller loops each, then the final exponentiations
zk_status enqueue_pairing(zk_vk* V, size_t n, const VerifyPlan& pl) {
    const uint32_t *a = V->aff_g1.as<const uint32_t>(), *c = a + n * 24, *acc = V->acc.as<const uint32_t>();
    const uint32_t *skip = V->skip.as<const uint32_t>(), *valid = V->valid.as<const uint32_t>(), *gam = V->gam.as<const uint32_t>();
    const uint32_t* prep_gamma = V->gamma_inf ? nullptr : V->prep[0].as<const uint32_t>();
    const uint32_t* prep_delta = V->delta_inf ? nullptr : V->prep[1].as<const uint32_t>();
    const F12* alpha_beta = V->alpha_beta.as<const F12>();
    uint32_t* ok = V->ok.as<uint32_t>();
    const unsigned b64 = (unsigned)((n + 63) / 64), bw = (unsigned)((n + zkdev::W3_GROUPS - 1) / zkdev::W3_GROUPS);
    if (pl.pairing == VPairing::ROWS) ZK_TRY(ensure_lines28(V, g_stream));
    {
        ProfScope ps("verify_miller");
        if (pl.pairing == VPairing::ROWS)
            zkcoop::verify_miller(a, V->coop_stage.p, acc, V->gamma_inf ? nullptr : V->lines28[0].p, c, V->delta_inf ? nullptr : V->lines28[1].p, skip,
                                  V->f.p, (uint32_t)n, g_stream);
        else if (pl.pairing == VPairing::LANES18)
            ZK_LAUNCH_SYNC(zkdev::k_miller_loop_wide, dim3(bw, 3), dim3(zkdev::W3_THREADS), 0, g_stream, a, V->prep_b.as<const uint32_t>(), acc,
                           prep_gamma, c, prep_delta, skip, V->f.as<F12>(), (uint32_t)n);
        else
            ZK_LAUNCH(zkdev::k_miller_loop, dim3(b64, 3), dim3(64), 0, g_stream, a, V->aff_g2.as<const uint32_t>(), acc, prep_gamma, c, prep_delta, skip,
                      V->f.as<F12>(), (uint32_t)n);
    }
    {
        ProfScope ps("verify_final");
        if (pl.pairing == VPairing::ROWS)
            zkcoop::verify_final_exp(V->f.p, gam, V->alpha_beta.p, valid, ok, nullptr, (uint32_t)n, g_stream);
        else if (pl.pairing == VPairing::LANES18)
            ZK_LAUNCH_SYNC(zkdev::k_final_exp_wide, dim3(bw), dim3(zkdev::W3_THREADS), 0, g_stream, V->f.as<const F12>(), gam, alpha_beta, valid, ok,
                           (F12*)nullptr, (uint32_t)n);
        else
            ZK_LAUNCH(zkdev::k_final_exp, dim3(b64), dim3(64), 0, g_stream, V->f.as<const F12>(), gam, alpha_beta, valid, ok, (F12*)nullptr, (uint32_t)n);
    }
    return ZK_OK;
}

// own_proofs: A, B, C were computed by this library's prover a moment ago (the self-check of gen_proof): group elements
// by construction, as the in-memory Proof the reference hands to verify_proof in check_proof (confidential.rs:208-278,
// no deserialisation there) - no r-torsion test, which only a foreign byte string needs; own_affine: see stage_own_affine
zk_status verify_chunk(zk_vk* V, size_t n, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out, bool own_proofs,
                       const uint8_t* own_affine, const VerifyTunables& tun) {
    const uint32_t ni = V->n_ic - 1;
    if (!own_proofs) own_affine = nullptr;
    const VerifyPlan pl = verify_plan(n, ni, own_proofs, own_affine != nullptr, tun);
    Staged s(n, own_affine ? nullptr : proofs);
    // a point at infinity in A, B or C is what Proof::read refuses (x = y = 0 stands for it in the host's affine form)
    auto zero = [](const uint8_t* q, size_t len) { return std::all_of(q, q + len, [](uint8_t b) { return b == 0; }); };
    for (size_t i = 0; own_affine && i < n; i++) {
        const uint8_t* a = own_affine + i * OWN_AFFINE_BYTES;
        s.enc[i] = zero(a, 96) || zero(a + 96, 192) || zero(a + 288, 96);
    }
    std::vector<uint32_t> bad(n, 0), sc((size_t)n * ni * 8, 0);
    for (size_t i = 0; i < n; i++) {
        if (s.enc[i] || !inputs_canonical(inputs + i * ni * 32, ni)) {
            bad[i] = 1;
            s.f1[i] = s.f1[n + i] = s.f2[i] = 1;   // decode nothing; its scalars stay zero
        } else if (ni) {   // (no inputs: `sc` is empty, nothing to index - UBSan, round 4)
            memcpy(&sc[i * ni * 8], inputs + i * ni * 32, (size_t)ni * 32);
        }
    }
    ZK_TRY(upload_staged(V, n, s, &bad));
    ZK_TRY(upload(V->scal, sc.data(), sc.size() * 4));
    if (own_affine) ZK_TRY(stage_own_affine(V, n, own_affine));
    ZK_TRY(V->part.ensure((size_t)n * (ni ? 16 * ni : 1) * sizeof(DG1)));   // (sixteen pieces per scalar from INPUTS_FINE_MIN proofs)
    ZK_TRY(V->acc.ensure(n * 96));
    ZK_TRY(V->acc_inf.ensure(n * 4));
    ZK_TRY(V->skip.ensure(n * 4));
    ZK_TRY(V->valid.ensure(n * 4));
    ZK_TRY(V->f.ensure(3 * n * sizeof(F12)));   // one Miller function per pair
    ZK_TRY(V->ok.ensure(n * 4));
    // three independent bundles of serial chains - the G2 decoder, the G1 decoder, the input accumulator - side by side
    // on the lane's three streams (each is a few dozen waves; one after the other they were 60 % of a verification)
    ZK_TRY(V->streams.fork());
    ZK_TRY(enqueue_head(V, n, pl, g_stream, g_stream2));
    ZK_TRY(V->streams.side_done());
    ZK_TRY(enqueue_inputs(V, n, pl, g_copy_stream));
    ZK_TRY(V->streams.copy_done());
    ZK_TRY(V->streams.join());
    ZK_LAUNCH(zkdev::k_verify_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, V->st_g1.as<const uint32_t>(),
              V->st_g2.as<const uint32_t>(), V->acc_inf.as<const uint32_t>(), V->host_bad.as<const uint32_t>(), V->skip.as<uint32_t>(),
              V->valid.as<uint32_t>(), (uint32_t)n);
    ZK_TRY(enqueue_pairing(V, n, pl));
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> okv(n);
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(okv.data(), V->ok.p, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) ok_out[i] = okv[i] ? 1 : 0;
    return ZK_OK;
}

// The stages of the combined check (verify_chunk_rlc), each on the stream it is given.  Behind the decoder of A | C: both
// scaled by rho_i, the C's summed
zk_status rlc_enqueue_scale(zk_vk* V, size_t n, hipStream_t st) {
    typedef RlcWork::P32 P32;
    const uint32_t *aff_g1 = V->aff_g1.as<const uint32_t>(), *rho = V->rlc.rho.as<const uint32_t>();
    uint32_t* pts = V->rlc.pts.as<uint32_t>();
    P32 *c = V->rlc.c.as<P32>(), *csum = V->rlc.csum.as<P32>();
    const uint32_t nb1 = (uint32_t)((n + 255) / 256);
    ProfScope ps("verify_rlc_scale", st);
    ZK_LAUNCH(zkdev::k_rlc_scale, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, st, aff_g1, rho, pts, c, (uint32_t)n);
    ZK_LAUNCH_SYNC(zkdev::k_g1_sum, dim3(nb1), dim3(64), 0, st, V->rlc.c.as<const P32>(), (uint32_t)n, csum + 1);
    ZK_LAUNCH_SYNC(zkdev::k_g1_sum, dim3(1), dim3(64), 0, st, V->rlc.csum.as<const P32>() + 1, nb1, csum);
    return ZK_OK;
}
// What the product is compared with, e(alpha, beta)^S = e(alpha, beta)^(sum a_i) (e(alpha, beta)^lambda)^(sum b_i) over
// `nbits` bits, and the accumulator sum_j s_j ic_j
zk_status rlc_enqueue_want(zk_vk* V, uint32_t nbits, hipStream_t st) {
    ZK_TRY(ensure_rlc_ab_lambda(V, st));   // (ahead of the scope: its one-off is not a stage time)
    const DG1A* table = V->ic_table.as<const DG1A>();
    const uint32_t *s = V->rlc.s.as<const uint32_t>(), *exp = V->rlc.exp.as<const uint32_t>();
    const F12 *alpha_beta = V->alpha_beta.as<const F12>(), *ab_lambda = V->rlc.ab_lambda.as<const F12>();
    ProfScope ps("verify_inputs", st);
    ZK_LAUNCH_SYNC(zkdev::k_rlc_inputs, dim3(1), dim3(zkdev::RLC_IN_THREADS), 0, st, table, s, V->rlc.acc.as<DG1>(), V->n_ic);
    ZK_LAUNCH_SYNC(zkdev::k_f12_pow2_wide, dim3(1), dim3(zkdev::W3_THREADS), 0, st, alpha_beta, ab_lambda, exp, nbits, V->rlc.want.as<F12>());
    return ZK_OK;
}
// On the main stream, behind the others: the two shared points behind the rho_i A_i, the flags, the key's line tables behind
// the batch's (pairs n and n + 1), ONE Miller loop over the m = n + 2 pairs, the product of its m functions as a tree of
// groups of twelve, ONE final exponentiation
zk_status rlc_enqueue_pairing(zk_vk* V, size_t n) {
    const size_t m = n + 2;
    ZK_TRY(ensure_rlc_fe(V, g_stream));
    const uint32_t *st_g1 = V->st_g1.as<const uint32_t>(), *st_g2 = V->st_g2.as<const uint32_t>(), *host_bad = V->host_bad.as<const uint32_t>();
    const uint32_t *inf = V->rlc.inf.as<const uint32_t>(), *pts = V->rlc.pts.as<const uint32_t>(), *skip = V->skip.as<const uint32_t>();
    const uint32_t *prep_b = V->prep_b.as<const uint32_t>(), *gam = V->gam.as<const uint32_t>(), *none = nullptr;
    const F12 *fe = V->rlc.fe.as<const F12>(), *want = V->rlc.want.as<const F12>();
    uint32_t* key_lines = V->prep_b.as<uint32_t>() + n * COEF_WORDS;
    ZK_LAUNCH(zkdev::k_rlc_shared_points, dim3(1), dim3(64), 0, g_stream, V->rlc.acc.as<const DG1>(), V->rlc.csum.as<const RlcWork::P32>(),
              V->rlc.pts.as<uint32_t>(), V->rlc.inf.as<uint32_t>(), (uint32_t)n);
    ZK_LAUNCH(zkdev::k_rlc_flags, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, g_stream, st_g1, st_g2, host_bad, inf, V->skip.as<uint32_t>(),
              V->rlc.all.as<uint32_t>(), (uint32_t)n);
    HIP_TRY(hipMemcpyAsync(key_lines, V->prep[0].p, COEF_WORDS * 4, hipMemcpyDeviceToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(key_lines + COEF_WORDS, V->prep[1].p, COEF_WORDS * 4, hipMemcpyDeviceToDevice, g_stream));
    {
        ProfScope ps("verify_miller");
        ZK_LAUNCH_SYNC(zkdev::k_miller_loop_wide, dim3((unsigned)((m + zkdev::W3_GROUPS - 1) / zkdev::W3_GROUPS), 1), dim3(zkdev::W3_THREADS), 0,
                       g_stream, pts, prep_b, none, none, none, none, skip, V->f.as<F12>(), (uint32_t)m);
    }
    ProfScope ps("verify_final");
    const F12* src = V->f.as<const F12>();
    F12* half[2] = {V->rlc.prod.as<F12>(), V->rlc.prod.as<F12>() + RlcWork::prod_half(m)};
    int which = 0;
    for (uint32_t cnt = (uint32_t)m; cnt > 1; which ^= 1) {
        const uint32_t groups = (cnt + 11) / 12;
        F12* dst = groups == 1 ? V->rlc.fe.as<F12>() : half[which];   // (the last product: the final exponentiation's operand)
        ZK_LAUNCH_SYNC(zkdev::k_f12_prod_wide, dim3((groups + zkdev::W3_GROUPS - 1) / zkdev::W3_GROUPS), dim3(zkdev::W3_THREADS), 0, g_stream, src,
                       cnt, dst, groups);
        src = dst;
        cnt = groups;
    }
    ZK_LAUNCH_SYNC(zkdev::k_final_exp_wide, dim3(1), dim3(zkdev::W3_THREADS), 0, g_stream, fe, gam, want, none, V->ok.as<uint32_t>(), (F12*)nullptr, 1u);
    return ZK_OK;
}

// The whole chunk in ONE combined check (pairing.h, "Batch verification with a random linear combination"):
//   prod_i e(rho_i A_i, B_i) * e(sum_j s_j ic_j, -gamma) * e(sum_i rho_i C_i, -delta) == e(alpha, beta)^(sum_i rho_i)
// with rho_i = 128 bits of Blake2s(digest of the batch, i): the coefficients are fixed by the proofs and inputs they
// weigh (Fiat-Shamir), no randomness source is needed and a run can be repeated.  *decided = true: every proof of the
// chunk verifies (probability of a wrong accept 2^-128 per attempt).  *decided = false: a proof of the chunk is malformed
// or invalid, or the combined check failed - the caller runs the per-proof verifier, which names the culprits.
zk_status verify_chunk_rlc(zk_vk* V, size_t n, const uint8_t* proofs, const uint8_t* inputs, bool own_proofs, bool* decided,
                           const VerifyTunables& tun) {
    *decided = false;
    const uint32_t ni = V->n_ic - 1;
    if (V->gamma_inf || V->delta_inf || !ni) return ZK_OK;   // degenerate keys: the per-proof path knows them
    const Staged staged(n, proofs);
    const std::vector<uint32_t> bad(n, 0);
    for (size_t i = 0; i < n; i++)   // a refused encoding, an input that is not a canonical Fr: undecided, nothing hashed
        if (staged.enc[i] || !inputs_canonical(inputs + i * ni * 32, ni)) return ZK_OK;
    // (alive until the streams have been waited for: the pageable source of asynchronous copies, as staged and bad are)
    const zkrlc::Coefs co = zkrlc::coefs(V->key_digest, n, ni, proofs, inputs, host_threads(n, 16),
                                         [](unsigned nth, auto& work) { run_threads(nth, work); });
    const size_t m = n + 2;
    ZK_TRY(upload_staged(V, n, staged, &bad));
    ZK_TRY(V->rlc.reserve(n, V->n_ic));
    HIP_TRY(hipMemcpyAsync(V->rlc.rho.p, co.rho.data(), co.rho.size() * 4, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(V->rlc.s.p, co.s.data(), co.s.size() * 4, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(V->rlc.exp.p, co.exp, 32, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemsetAsync(V->rlc.all.p, 0xff, 4, g_stream));
    ZK_TRY(V->streams.fork());
    // the workspaces shared with the per-proof path, for the m pairs
    ZK_TRY(V->skip.ensure(m * 4));
    ZK_TRY(V->f.ensure(3 * m * sizeof(F12)));
    ZK_TRY(V->ok.ensure(4));
    ZK_TRY(V->prep_b.ensure(m * COEF_WORDS * 4));   // (the key's two tables behind the n of the batch: BEFORE enqueue_head reserves n)
    // main stream: B decoded, its lines prepared (the r-torsion test rides on the preparation); side stream: A and C decoded
    ZK_TRY(enqueue_head(V, n, verify_plan_lane_head(n, own_proofs, tun, true), g_stream, g_stream2));
    ZK_TRY(rlc_enqueue_scale(V, n, g_stream2));
    ZK_TRY(V->streams.side_done());
    ZK_TRY(rlc_enqueue_want(V, co.nbits, g_copy_stream));
    ZK_TRY(V->streams.copy_done());
    ZK_TRY(V->streams.join());
    ZK_TRY(rlc_enqueue_pairing(V, n));
    HIP_TRY(hipGetLastError());
    uint32_t okv = 0, allv = 0;
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(&okv, V->ok.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&allv, V->rlc.all.p, 4, hipMemcpyDeviceToHost));
    *decided = okv == 1 && allv != 0;
    if (hook_env("ZKAMD_DEBUG_RLC"))   // tests: was the chunk really decided by the combined check?
        fprintf(stderr, "[rlc] chunk of %zu proofs: combined check %s, every proof well-formed: %s\n", n, okv == 1 ? "passed" : "FAILED",
                allv ? "yes" : "NO");
    return ZK_OK;
}

}  // namespace

namespace zkrt {
// the random-linear-combination check first (verify_chunk_rlc) on the chunks verify_plan.h names for it, the per-proof
// verifier for the others and for a chunk the combined check cannot vouch for
zk_status verify_batch(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs, uint8_t* ok_out,
                       bool own_proofs, int form, const uint8_t* own_affine) {
    if (!vk || (n && (!proofs || !ok_out)) || (n && n_inputs && !public_inputs)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    // verifier.rs:38-40
    if (n_inputs + 1 != vk->ic.size()) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "number of public inputs + 1 differs from ic");
    ZK_TRY(use_device(vk->device));
    for (size_t first = 0; first < n; first += VERIFY_CHUNK) {
        const size_t np = std::min(VERIFY_CHUNK, n - first);
        const VerifyTunables tun = VerifyTunables::read();
        if (verify_takes_combined(form, np, tun)) {
            bool decided = false;
            ZK_TRY(verify_chunk_rlc(vk, np, proofs + first * 192, public_inputs + first * n_inputs * 32, own_proofs, &decided, tun));
            if (decided) {
                memset(ok_out + first, 1, np);
                continue;
            }
        }
        ZK_TRY(verify_chunk(vk, np, proofs + first * 192, public_inputs + first * n_inputs * 32, ok_out + first, own_proofs,
                            own_affine ? own_affine + first * OWN_AFFINE_BYTES : nullptr, tun));
    }
    return ZK_OK;
}
}  // namespace zkrt

namespace {
// verify_confidential_proof / verify_anonymous_proof (modules/zk-system/src/lib.rs:56-165) for n extrinsics: the n_fields
// points of each, in the reference's push order, through IntoXY (xt_inputs.h), then verify_batch.  field(i, k): the encoding
// of field k = 1 .. n_fields of extrinsic i; with a shared g_epoch (stride 0) that one encoding is decoded once.
template <class Xt, class Field>
zk_status xt_verify_batch(zk_vk* vk, size_t n, const Xt* xts, const uint8_t* g_epochs, size_t g_epoch_stride, uint8_t* ok_out,
                          uint8_t* refusal_out, size_t n_fields, size_t epoch_field, Field field) {
    if (!vk) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (vk->ic.size() != 2 * n_fields + 1)
        return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "the key does not have " + std::to_string(2 * n_fields) + " public inputs");
    if (!n) return ZK_OK;
    if (!xts || !g_epochs || !ok_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (g_epoch_stride != 0 && g_epoch_stride != 32) return fail(ZK_ERR_INVALID_ARGUMENT, "g_epoch_stride must be 0 or 32");
    const bool shared = g_epoch_stride == 0;
    const size_t per = n_fields - (shared ? 1 : 0);
    for (size_t first = 0; first < n; first += VERIFY_CHUNK) {
        const size_t np = std::min(VERIFY_CHUNK, n - first), total = np * per + (shared ? 1 : 0);
        std::vector<uint8_t> pts(total * 32), xy(total * 64), st(total), proofs(np * 192), inputs(np * n_fields * 64, 0), refusal(np, 0);
        size_t at = 0;
        if (shared) memcpy(&pts[32 * at++], g_epochs, 32);
        for (size_t i = 0; i < np; i++) {
            memcpy(&proofs[i * 192], xts[first + i].proof, 192);
            for (size_t k = 1; k <= n_fields; k++)
                if (!(shared && k == epoch_field)) memcpy(&pts[32 * at++], field(first + i, k), 32);
        }
        ZK_TRY(zkxt::into_xy(pts.data(), total, vk->device, &vk->xt, xy.data(), st.data()));
        at = shared ? 1 : 0;
        for (size_t i = 0; i < np; i++) {
            uint8_t* row = &inputs[i * n_fields * 64];
            for (size_t k = 1; k <= n_fields; k++) {
                const size_t idx = shared && k == epoch_field ? 0 : at++;
                if (st[idx] && !refusal[i]) refusal[i] = (uint8_t)(k | ((size_t)st[idx] << 6));
                memcpy(row + (k - 1) * 64, &xy[idx * 64], 64);
            }
            if (refusal[i]) memset(row, 0, n_fields * 64);   // the reference never reaches verify_proof with it
        }
        ZK_TRY(zkrt::verify_batch(vk, np, proofs.data(), inputs.data(), 2 * n_fields, ok_out + first, false, zkrt::VERIFY_AUTO, nullptr));
        for (size_t i = 0; i < np; i++) {
            if (refusal[i]) ok_out[first + i] = 0;
            if (refusal_out) refusal_out[first + i] = refusal[i];
        }
    }
    return ZK_OK;
}
}  // namespace

extern "C" {

zk_status zk_vk_prepare(const uint8_t* vk_bytes, size_t len, int device, zk_vk** out) try {
    if (!vk_bytes || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return vk_prepare(vk_bytes, len, device, out);
} ZK_ABI_CATCH
zk_status zk_vk_read(const uint8_t* pvk_bytes, size_t len, int device, zk_vk** out) try {
    if (!pvk_bytes || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return vk_read_prepared(pvk_bytes, len, device, out);
} ZK_ABI_CATCH
zk_status zk_vk_write(const zk_vk* vk, uint8_t* out, size_t cap, size_t* len) try {
    if (!vk || !len) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<uint8_t> o;
    zkhost::Fq2 c;
    for (int i = 0; i < 6; i++) {
        memcpy(&c, &vk->h_alpha_beta[i * 24], 96);
        fq2_write(o, c);
    }
    for (int k = 0; k < 2; k++) {
        const bool inf = k == 0 ? vk->gamma_inf : vk->delta_inf;
        const uint32_t cnt = inf ? 0u : (uint32_t)zkdev::PAIRING_NCOEF;
        put_u32be(o, cnt);
        for (uint32_t i = 0; i < cnt * 3; i++) {
            memcpy(&c, &vk->h_prep[k][(size_t)i * 24], 96);
            fq2_write(o, c);
        }
        o.push_back(inf ? 1 : 0);
    }
    put_u32be(o, (uint32_t)vk->ic.size());
    for (const HG1A& p : vk->ic) {
        uint8_t b[96];
        zkhost::g1_to_uncompressed(p, b);
        o.insert(o.end(), b, b + 96);
    }
    *len = o.size();
    if (out) {
        if (cap < o.size()) return fail(ZK_ERR_INVALID_ARGUMENT, "output buffer too small");
        memcpy(out, o.data(), o.size());
    }
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_vk_num_inputs(const zk_vk* vk, uint32_t* n_inputs) try {
    if (!vk || !n_inputs) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    *n_inputs = vk->n_ic ? vk->n_ic - 1 : 0;
    return ZK_OK;
} ZK_ABI_CATCH
void zk_vk_free(zk_vk* vk) { delete vk; }

zk_status zk_verify_batch(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs,
                          uint8_t* ok_out) try {
    return zkrt::verify_batch(vk, n, proofs, public_inputs, n_inputs, ok_out, false, zkrt::VERIFY_AUTO, nullptr);
} ZK_ABI_CATCH
zk_status zk_verify_batch_rlc(zk_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_inputs,
                              uint8_t* ok_out) try {
    return zkrt::verify_batch(vk, n, proofs, public_inputs, n_inputs, ok_out, false, zkrt::VERIFY_COMBINED, nullptr);
} ZK_ABI_CATCH
zk_status zk_proof_read_batch(zk_vk* vk, size_t n, const uint8_t* proofs, uint8_t* status_out) try {
    if (!vk || (n && (!proofs || !status_out))) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(vk->device));
    for (size_t first = 0; first < n; first += VERIFY_CHUNK) {
        const size_t np = std::min(VERIFY_CHUNK, n - first);
        const uint8_t* pr = proofs + first * 192;
        const Staged s(np, pr);
        ZK_TRY(upload_staged(vk, np, s, nullptr));
        // B as zk_verify_batch treats it: the reader reports what the verifier would act on
        ZK_TRY(enqueue_head(vk, np, verify_plan_lane_head(np, false, VerifyTunables::read(), false), g_stream, g_stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g_stream));
        std::vector<uint32_t> s1(2 * np), s2(np);
        HIP_TRY(hipMemcpy(s1.data(), vk->st_g1.p, 2 * np * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(s2.data(), vk->st_g2.p, np * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < np; i++) {
            uint8_t st = 0;
            // the order Proof::read meets them in: A, B, C, each point completely before the next
            // (core/bellman-verifier/src/lib.rs:67-110): bad encoding, then the decoder's verdict on that point
            const uint32_t d[3] = {s1[i], s2[i], s1[np + i]};
            for (int k = 0; k < 3 && !st; k++) {
                if (s.enc[i] & (1u << k))
                    st = (uint8_t)((k + 1) | (ZK_PROOF_BAD_ENCODING << 2));
                else if (d[k])   // decoder states 1 / 2 / 3 = not on the curve / not in the subgroup / infinity
                    st = (uint8_t)((k + 1) | ((d[k] == 1 ? ZK_PROOF_NOT_ON_CURVE : d[k] == 2 ? ZK_PROOF_NOT_IN_SUBGROUP : ZK_PROOF_INFINITY) << 2));
            }
            status_out[first + i] = st;
        }
    }
    return ZK_OK;
} ZK_ABI_CATCH
zk_status zk_verify_proof(zk_vk* vk, const uint8_t proof[192], const uint8_t* public_inputs, size_t n_inputs, int* ok) try {
    if (!ok) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    uint8_t v = 0;
    zk_status st = zk_verify_batch(vk, 1, proof, public_inputs, n_inputs, &v);
    *ok = v;
    return st;
} ZK_ABI_CATCH

zk_status zk_jubjub_into_xy(const uint8_t* points, size_t n, int device, uint8_t* xy_out, uint8_t* status_out) try {
    if (n && (!points || !xy_out || !status_out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return zkxt::into_xy(points, n, device, nullptr, xy_out, status_out);
} ZK_ABI_CATCH
zk_status zk_elgamal_ledger_apply(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, int device, uint8_t* slots_out,
                                  uint8_t* before_out, uint8_t* slot_status_out, uint8_t* op_status_out) try {
    return zkledger::apply(n_slots, slots, n_ops, ops, device, slots_out, before_out, slot_status_out, op_status_out);
} ZK_ABI_CATCH
zk_status zk_confidential_verify_batch(zk_vk* vk, size_t n, const zk_confidential_xt* xts, const uint8_t* enc_balances,
                                       const uint8_t* g_epochs, size_t g_epoch_stride, uint8_t* ok_out, uint8_t* refusal_out) try {
    auto field = [&](size_t i, size_t k) -> const uint8_t* {
        const zk_confidential_xt& x = xts[i];
        const uint8_t* bal = enc_balances ? enc_balances + i * 64 : x.enc_balance;
        switch (k) {
            case 1: return x.enc_key_sender;
            case 2: return x.enc_key_recipient;
            case 3: return x.left_amount_sender;
            case 4: return x.left_amount_recipient;
            case 5: return x.right_randomness;
            case 6: return x.left_fee;
            case 7: return bal;
            case 8: return bal + 32;
            case 9: return x.rvk;
            case 10: return g_epochs + i * g_epoch_stride;
            default: return x.nonce;
        }
    };
    return xt_verify_batch(vk, n, xts, g_epochs, g_epoch_stride, ok_out, refusal_out, 11, 10, field);
} ZK_ABI_CATCH
zk_status zk_anonymous_verify_batch(zk_vk* vk, size_t n, const zk_anonymous_xt* xts, const uint8_t* enc_balances,
                                    const uint8_t* g_epochs, size_t g_epoch_stride, uint8_t* ok_out, uint8_t* refusal_out) try {
    if (n && !enc_balances) return fail(ZK_ERR_INVALID_ARGUMENT, "enc_balances is required");
    auto field = [&](size_t i, size_t k) -> const uint8_t* {
        const zk_anonymous_xt& x = xts[i];
        const size_t S = ZK_ANONYMOUS_SIZE;
        if (k <= S) return x.enc_keys[k - 1];
        if (k <= 2 * S) return x.left_ciphertexts[k - 1 - S];
        if (k <= 3 * S) return enc_balances + (i * S + (k - 1 - 2 * S)) * 64;
        if (k <= 4 * S) return enc_balances + (i * S + (k - 1 - 3 * S)) * 64 + 32;
        switch (k - 4 * S) {
            case 1: return x.right_ciphertext;
            case 2: return x.rvk;
            case 3: return g_epochs + i * g_epoch_stride;
            default: return x.nonce;
        }
    };
    return xt_verify_batch(vk, n, xts, g_epochs, g_epoch_stride, ok_out, refusal_out, 4 * ZK_ANONYMOUS_SIZE + 4, 4 * ZK_ANONYMOUS_SIZE + 3, field);
} ZK_ABI_CATCH
zk_status zk_confidential_block_execute(zk_vk* vk, size_t n, const zk_confidential_xt* xts, const uint8_t* sigs, const uint8_t* msgs,
                                        const uint64_t* msg_offsets, size_t n_accounts, const zk_block_account* accounts, size_t n_pool,
                                        const uint8_t* nonce_pool, const uint8_t g_epoch[32], zk_block_account* accounts_out,
                                        zk_block_verdict* verdicts_out, zk_block_stats* stats_out) try {
    if (!vk) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (vk->ic.size() != 2 * zkblock::XT_FIELDS + 1) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "the key does not have 22 public inputs");
    vk->block.is_public = true;
    auto verify = [&](size_t nv, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok) {
        return zkrt::verify_batch(vk, nv, proofs, inputs, 2 * zkblock::XT_FIELDS, ok, false, zkrt::VERIFY_AUTO, nullptr);
    };
    const zkblock::BlockArgs A{vk->device, &vk->xt,    &vk->block, &vk->block_rows, n,       sigs,         msgs,         msg_offsets,
                               n_accounts, accounts,   n_pool,     nonce_pool,      g_epoch, accounts_out, verdicts_out, stats_out};
    return zkblock::execute(A, verify, xts);
} ZK_ABI_CATCH
zk_status zk_anonymous_block_execute(zk_vk* vk, size_t n, const zk_anonymous_xt* xts, const uint8_t* sigs, const uint8_t* msgs,
                                     const uint64_t* msg_offsets, size_t n_accounts, const zk_block_account* accounts, size_t n_pool,
                                     const uint8_t* nonce_pool, const uint8_t g_epoch[32], zk_block_account* accounts_out,
                                     zk_block_verdict* verdicts_out, zk_block_stats* stats_out) try {
    if (!vk) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (vk->ic.size() != 2 * zkblock::AX_FIELDS + 1) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "the key does not have 104 public inputs");
    vk->block.is_public = true;
    auto verify = [&](size_t nv, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok) {
        return zkrt::verify_batch(vk, nv, proofs, inputs, 2 * zkblock::AX_FIELDS, ok, false, zkrt::VERIFY_AUTO, nullptr);
    };
    const zkblock::BlockArgs A{vk->device, &vk->xt,    &vk->block, &vk->block_rows, n,       sigs,         msgs,         msg_offsets,
                               n_accounts, accounts,   n_pool,     nonce_pool,      g_epoch, accounts_out, verdicts_out, stats_out};
    return zkblock::execute_anonymous(A, verify, xts);
} ZK_ABI_CATCH
zk_status zk_asset_block_execute(zk_vk* vk, size_t n, const zk_confidential_xt* xts, const uint8_t* kinds, const uint32_t* asset_ids, const uint8_t* sigs,
                                 const uint8_t* msgs, const uint64_t* msg_offsets, size_t n_accounts, const zk_block_account* accounts,
                                 const uint32_t* account_asset_ids, size_t n_pool, const uint8_t* nonce_pool, const uint8_t g_epoch[32],
                                 uint32_t next_asset_id, zk_block_account* accounts_out, zk_block_verdict* verdicts_out, zk_asset_effect* effects_out,
                                 uint32_t* next_asset_id_out, zk_block_stats* stats_out) try {
    if (!vk) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (vk->ic.size() != 2 * zkblock::XT_FIELDS + 1) return fail(ZK_ERR_MALFORMED_VERIFYING_KEY, "the key does not have 22 public inputs");
    vk->block.is_public = true;
    auto verify = [&](size_t nv, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok) {
        return zkrt::verify_batch(vk, nv, proofs, inputs, 2 * zkblock::XT_FIELDS, ok, false, zkrt::VERIFY_AUTO, nullptr);
    };
    const zkblock::BlockArgs A{vk->device, &vk->xt,    &vk->block, &vk->block_rows, n,       sigs,         msgs,         msg_offsets,
                               n_accounts, accounts,   n_pool,     nonce_pool,      g_epoch, accounts_out, verdicts_out, stats_out};
    return zkblock::execute_asset(A, verify, xts, kinds, asset_ids, account_asset_ids, next_asset_id, effects_out, next_asset_id_out);
} ZK_ABI_CATCH
zk_status zk_g_epoch(uint32_t epoch, uint8_t out[32]) try {
    if (!out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    return zkblock::g_epoch(epoch, out);
} ZK_ABI_CATCH

#ifdef ZK_TEST_HOOKS
// Test hook, NOT part of the ABI (absent from libzkamd.so): 1 / x for n field elements of Fq in the host's Montgomery words,
// through the inversion routine of the verification kernels on rows (coop_inv.h).
zk_status zk_hook_fq_inverse(const uint32_t* in, uint32_t* out, size_t n) try {
    if (!in || !out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    ZK_TRY(use_device(0));
    DevBuf a, b;
    a.is_public = b.is_public = true;
    ZK_TRY(a.ensure(n * 48));
    ZK_TRY(b.ensure(n * 48));
    HIP_TRY(hipMemcpy(a.p, in, n * 48, hipMemcpyHostToDevice));
    zkcoop::test_inverse((const uint32_t*)a.p, (uint32_t*)b.p, (uint32_t)n, g_stream);
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(out, b.p, n * 48, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH
// ... and the plan of a chunk of n proofs (verify_plan.h) under the environment of the call, no GPU involved: out[0 .. 9) =
// the fields of VerifyPlan in their order, the enumerators as numbers, then whether verify_batch tries the combined check first
zk_status zk_hook_verify_plan(size_t n, size_t n_inputs, int own_proofs, int have_own_affine, int form, uint64_t* out, size_t out_words) try {
    if (!out || out_words < 9) return fail(ZK_ERR_INVALID_ARGUMENT, "output too short");
    const VerifyTunables tun = VerifyTunables::read();
    const VerifyPlan p = verify_plan(n, n_inputs, own_proofs != 0, have_own_affine != 0, tun);
    const uint64_t f[9] = {(uint64_t)p.decode, p.b_torsion_in_decoder, p.subgroup_tests, (uint64_t)p.prepare, p.prep_b_points, (uint64_t)p.inputs,
                           p.inputs_mul, (uint64_t)p.pairing, verify_takes_combined(form, n, tun)};
    std::copy(f, f + 9, out);
    return ZK_OK;
} ZK_ABI_CATCH
// ... and the coefficients of the combined check of a chunk (verify_rlc.h) on `threads` host threads, no GPU involved: rho_out
// 16 n bytes, s_out 32 (n_inputs + 1), exp_out 32
zk_status zk_hook_rlc_coefs(const uint8_t key_digest[32], size_t n, size_t n_inputs, const uint8_t* proofs, const uint8_t* inputs, unsigned threads,
                            uint8_t* rho_out, uint8_t* s_out, uint8_t* exp_out, uint32_t* nbits_out) try {
    if (!key_digest || !n || !proofs || (n_inputs && !inputs) || !rho_out || !s_out || !exp_out || !nbits_out)
        return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    const zkrlc::Coefs co =
        zkrlc::coefs(key_digest, n, (uint32_t)n_inputs, proofs, inputs, threads, [](unsigned nth, auto& work) { run_threads(nth, work); });
    memcpy(rho_out, co.rho.data(), co.rho.size() * 4);
    memcpy(s_out, co.s.data(), co.s.size() * 4);
    memcpy(exp_out, co.exp, 32);
    *nbits_out = co.nbits;
    return ZK_OK;
} ZK_ABI_CATCH
// ... and zk_elgamal_ledger_apply's arguments through the scan that can forget (asset_block_exec.h): flag bit 2 is LEDGER_CLEAR,
// the four k_asset_* kernels always run
zk_status zk_hook_ledger_apply_clear(size_t n_slots, const uint8_t* slots, size_t n_ops, const zk_ledger_op* ops, int device, uint8_t* slots_out,
                                     uint8_t* before_out, uint8_t* slot_status_out, uint8_t* op_status_out) try {
    return zkblock::apply_clear(n_slots, slots, n_ops, ops, device, slots_out, before_out, slot_status_out, op_status_out);
} ZK_ABI_CATCH
#endif

}  // extern "C"
