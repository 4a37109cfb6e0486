// IntoXY for a batch of Jubjub encodings: the public inputs of a transfer extrinsic from its bytes.
//
// PublicInputBuilder::push (modules/zk-system/src/input_builder.rs:15-27) calls IntoXY on every point of an extrinsic
// (core/primitives/src/{enc_key,left_ciphertext,right_ciphertext,nonce,g_epoch,sig_vk}.rs): edwards::Point::read
// (core/jubjub/src/curve/edwards.rs:92-165: y with the sign of x in the top bit, x by a square root in Fr), as_prime_order
// (:319-330: [s]P == O for the order s of the prime-order subgroup) and the affine pair (x, y) - two consecutive public
// inputs of verify_proof.  Eleven points per confidential transfer, fifty-two per anonymous one.
//
// Two forms, the same bytes:
//   host    zkwit::decode_point + zkwit::is_prime_order (transfer_witness.h) on the zk_set_host_threads pool
//   device  k_into_xy, one lane per point.  A point is one serial chain of Fr products and the chain is the whole cost
//           (11 264 lanes of a 1024-transfer block are a sixth of the machine at one wave per SIMD), so the kernel is built to
//           keep it short (2.55 ms for the 11 264 points of 1024 transfers, against 61 ms on 16 host threads) - about 3 200
//           dependent products per point where the witness kernels' decode_point / is_prime_order
//           pair (witness_gpu.h) takes about 4 500:
//             1 / (d y^2 + 1)   one exponentiation by r - 2 in fixed 4-bit windows                    ~330
//             square root       ONE exponentiation w = a^((q - 1) / 2), r - 1 = 2^32 q, in 4-bit windows; x = a w, b = x w
//                               = a^q; Tonelli-Shanks on b; existence decided by x^2 == a at the end   ~290 + <= 500
//             [s]P              s recoded at compile time into signed digits +-1, +-3, +-5, +-7 (width-4 NAF: 252
//                               doublings, 51 additions); doubling dbl-2008-hwcd for a = -1 (4M + 4S, 3M + 4S where T is
//                               not read); additions against P, 3P, 5P, 7P cached as (Y + X, Y - X, 2 d T, 2 Z): 7M  ~2 200
//           The two window tables (a^1 .. a^15; the four cached multiples) live in LDS, [slot][word][lane]: 32 KB per
//           64-lane block, every lane in its own bank, nothing in scratch memory.
// The chain's pieces (Lds, pow_windows, sqrt_one_pow, the Edwards steps, is_prime_order, read_point) are jubjub_dev.h's; this
// header holds the kernel and its host side, and only verify.cpp includes it: the library carries ONE k_into_xy.
// The inputs are public: nothing here is constant-time, and the buffers are freed without the wipe.
#pragma once
#include "jubjub_dev.h"
#include "host_common.h"
#include "host_math.h"
#include "transfer_witness.h"

namespace zkxt {

using zkrt::fail;

// ZKAMD_INTO_XY_HOST_MAX: points up to which the host form runs.  Measured crossover (profiles/r10_xt_verify_probe.json, 16 host
// threads): the kernel is 2.55-2.65 ms whatever the batch holds, the host form 1.84 ms at 256 points and 4.22 ms at 704.
constexpr size_t INTO_XY_HOST_MAX = 384;

// enc: n x 8 words.  xy: n x 16 words, x then y, plain little-endian canonical; zero where refused.  status: n words.
static __global__ void __launch_bounds__(64)
k_into_xy(const uint32_t* enc, uint32_t* xy, uint32_t* status, uint32_t n) {
    ZK_SHARED uint32_t table[16 * 8 * 64];
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const Lds L{table + threadIdx.x};
    Fr x, y, xm, ym, d;
    uint32_t st = read_point(L, enc + (size_t)t * 8, &x, &y, &xm, &ym, &d);
    if (st == INTO_XY_OK && !is_prime_order(L, xm, ym, dbl(d))) st = INTO_XY_NOT_PRIME_ORDER;
    if (st != INTO_XY_OK) x = y = Fr::zero();
    uint4* o = reinterpret_cast<uint4*>(xy + (size_t)t * 16);
    o[0] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
    o[1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    o[2] = make_uint4(y.l[0], y.l[1], y.l[2], y.l[3]);
    o[3] = make_uint4(y.l[4], y.l[5], y.l[6], y.l[7]);
    status[t] = st;
}

// ---- host form: decode_prime_order's arithmetic, one point
inline uint8_t into_xy_one(const uint8_t b[32], uint8_t xy[64]) {
    memset(xy, 0, 64);
    uint64_t v[4];
    zkrt::load_scalar_le(b, v);
    v[3] &= 0x7fffffffffffffffull;
    if (zkhost::Fr::geq_p(v)) return INTO_XY_NOT_IN_FIELD;
    zkwit::JPoint p;
    if (!zkwit::decode_point(b, &p)) return INTO_XY_NOT_ON_CURVE;
    if (!zkwit::is_prime_order(p)) return INTO_XY_NOT_PRIME_ORDER;
    const zkhost::Fr x = p.x.from_mont(), y = p.y.from_mont();
    memcpy(xy, x.l, 32);
    memcpy(xy + 32, y.l, 32);
    return INTO_XY_OK;
}

// the one reader of ZKAMD_INTO_XY_HOST_MAX (per call): zk_jubjub_into_xy, zk_elgamal_ledger_apply and the block executors
inline size_t into_xy_host_max() {
    const char* e = getenv("ZKAMD_INTO_XY_HOST_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : INTO_XY_HOST_MAX;
}

// The host form for callers that go on computing: the n encodings enc_of(0 .. n - 1) on the host threads, the status and the
// point in Montgomery form of each (x = y = 0 where refused)
template <class EncOf>
inline void into_xy_points(size_t n, EncOf&& enc_of, uint32_t* st, zkwit::JPoint* pt) {
    const unsigned nth = zkrt::host_threads(n, 64);
    auto work = [&](unsigned t) {
        for (size_t p = n * t / nth; p < n * (t + 1) / nth; p++) {
            uint8_t xy[64];
            st[p] = into_xy_one(enc_of(p), xy);
            zkhost::Fr x, y;
            memcpy(x.l, xy, 32);
            memcpy(y.l, xy + 32, 32);
            pt[p] = zkwit::JPoint{x.to_mont(), y.to_mont()};
        }
    };
    zkrt::run_threads(nth, work);
}

// the workspaces of the device form (public data: no wipe)
struct IntoXyBufs {
    zkrt::DevBuf in, out;
    IntoXyBufs() { in.is_public = out.is_public = true; }
};

// IntoXY for n encodings (zk_jubjub_into_xy).  device < 0, or n <= ZKAMD_INTO_XY_HOST_MAX (read per call; 0 = always the
// device form): the host form.  Else the kernel on the library stream of `device`, coordinates and statuses back in one copy.
inline zk_status into_xy(const uint8_t* points, size_t n, int device, IntoXyBufs* bufs, uint8_t* xy_out, uint8_t* status_out) {
    if (!n) return ZK_OK;
    if (device < 0 || n <= into_xy_host_max()) {
        const unsigned nth = zkrt::host_threads(n, 64);
        auto work = [&](unsigned t) {
            for (size_t i = n * t / nth; i < n * (t + 1) / nth; i++) status_out[i] = into_xy_one(points + i * 32, xy_out + i * 64);
        };
        zkrt::run_threads(nth, work);
        return ZK_OK;
    }
    ZK_TRY(zkrt::use_device(device));
    IntoXyBufs local;
    if (!bufs) bufs = &local;
    constexpr size_t SLICE = (size_t)1 << 20;   // points per launch
    std::vector<uint32_t> back;
    for (size_t first = 0; first < n; first += SLICE) {
        const size_t np = std::min(SLICE, n - first);
        ZK_TRY(bufs->in.ensure(np * 32));
        ZK_TRY(bufs->out.ensure(np * 68));
        HIP_TRY(hipMemcpyAsync(bufs->in.p, points + first * 32, np * 32, hipMemcpyHostToDevice, zkrt::g_stream));
        uint32_t* d_xy = bufs->out.as<uint32_t>();
        {
            zkrt::ProfScope ps("into_xy");
            ZK_LAUNCH(k_into_xy, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, zkrt::g_stream, (const uint32_t*)bufs->in.as<uint32_t>(), d_xy,
                      d_xy + np * 16, (uint32_t)np);
        }
        HIP_TRY(hipGetLastError());
        back.resize(np * 17);
        HIP_TRY(hipMemcpyAsync(back.data(), bufs->out.p, np * 68, hipMemcpyDeviceToHost, zkrt::g_stream));
        HIP_TRY(hipStreamSynchronize(zkrt::g_stream));
        memcpy(xy_out + first * 64, back.data(), np * 64);
        for (size_t i = 0; i < np; i++) status_out[first + i] = (uint8_t)back[np * 16 + i];
    }
    return ZK_OK;
}

// The device form alone, nothing copied back (ledger.h): the n encodings through k_into_xy in one launch on the library stream
// of the device in use.  bufs->out then holds n x 16 coordinate words and, behind them, n status words; in_extra / out_extra
// bytes are reserved behind the encodings and behind the statuses (from INTO_XY_OUT_ALIGN up) for what the caller keeps there.
constexpr size_t INTO_XY_OUT_ALIGN = 16;
inline size_t into_xy_out_bytes(size_t n) { return (n * 68 + INTO_XY_OUT_ALIGN - 1) / INTO_XY_OUT_ALIGN * INTO_XY_OUT_ALIGN; }
inline zk_status into_xy_on_device(const uint8_t* points, size_t n, IntoXyBufs* bufs, size_t in_extra, size_t out_extra) {
    if (n > (size_t)1 << 30) return fail(ZK_ERR_INVALID_ARGUMENT, "more than 2^30 points in one call");
    ZK_TRY(bufs->in.ensure(n * 32 + in_extra));
    ZK_TRY(bufs->out.ensure(into_xy_out_bytes(n) + out_extra));
    if (!n) return ZK_OK;
    HIP_TRY(hipMemcpyAsync(bufs->in.p, points, n * 32, hipMemcpyHostToDevice, zkrt::g_stream));
    uint32_t* d_xy = bufs->out.as<uint32_t>();
    zkrt::ProfScope ps("into_xy");
    ZK_LAUNCH(k_into_xy, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, zkrt::g_stream, (const uint32_t*)bufs->in.as<uint32_t>(), d_xy, d_xy + n * 16,
              (uint32_t)n);
    return ZK_OK;
}

}  // namespace zkxt
