// The plan of one chain of k_ntt_pass launches (zkamd.cpp NttPlan::chain): which tile form a transform takes, how its k
// stages are cut into passes, and the block, grid and LDS bytes of every pass - pure integer arithmetic on (k, batch, the
// form), nothing here touches the HIP runtime, so the CPU suite pins the launches of the product (tests/test_ntt_passes.py,
// through zk_hook_ntt_plan).  Every form gives the same bytes, so a threshold that moves by accident passes every parity
// test: it is pinned here.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "ntt.h"

namespace zkrt {

using zkdev::NttPass;

// The tile forms of k_ntt_pass:
//   latency   2^8-element tiles, one butterfly per thread and stage (a handful of small transforms: the H pipeline of a proof
//             made alone - 2^15 elements, 32 workgroups of 2^10-element tiles, every thread four butterflies per stage one after
//             the other, 25 us per pass on a machine that is otherwise idle; this form: four times the workgroups, ~10 us per
//             pass, the 32-byte segments of its strided pass come out of L2)
//   small     2^10-element tiles (32 KiB of LDS, 256 threads), up to 8 stages per pass: the in-step transforms
//   mid       2^11-element tiles (64 KiB of LDS, 512 threads), two workgroups per CU; the pass whose tile is contiguous takes 11
//             stages, the strided ones up to 9 (four columns = 128-byte segments): 2^20 in two passes.  Pair of transforms, ms:
//             2^17 0.228 -> 0.140, 2^18 0.245 -> 0.155, 2^20 0.288 -> 0.279, 2^22 1.349 -> 1.166 against `big`
//             (profiles/r06q_ntt_tiles.txt; VERDICT r5 item 4 asked <= 0.27)
//   big       2^12-element tiles (128 KiB, 1024 threads), one workgroup per CU, 10 stages per pass (rounds 2-5)
enum NttForm : int { NTT_FORM_LATENCY = 0, NTT_FORM_SMALL = 1, NTT_FORM_MID = 2, NTT_FORM_BIG = 3 };

constexpr uint32_t NTT_MAX_LOG = 27;          // the largest domain (NttPlan::init)
constexpr uint32_t NTT_LDS_MAX = 160 * 1024;  // dynamic LDS a workgroup may ask for on gfx950

// ZKAMD_NTT_TILES = mid | big | small: the tile form of the transforms of 2^17 and more (mid by default, round 6; A/B)
inline NttForm ntt_tiles(const char* env) {
    return !env ? NTT_FORM_MID : !strcmp(env, "big") ? NTT_FORM_BIG : !strcmp(env, "small") ? NTT_FORM_SMALL : NTT_FORM_MID;
}

// the latency form: chosen per chain by the batch's size
inline bool ntt_latency_form(uint32_t k, uint32_t batch) {
    return k >= 9 && k < (uint32_t)zkdev::NTT_BIG_LOG && ((uint64_t)batch << k) <= (1u << 17);
}

// The form the product takes for a chain of `batch` transforms of 2^k under the tile choice `tiles` (ntt_tiles).
inline NttForm ntt_form(NttForm tiles, uint32_t k, uint32_t batch) {
    if (ntt_latency_form(k, batch)) return NTT_FORM_LATENCY;
    return k >= (uint32_t)zkdev::NTT_BIG_LOG && tiles != NTT_FORM_LATENCY ? tiles : NTT_FORM_SMALL;
}

// Whether a form can be built for a size: the contiguous pass of `mid` alone has 11 stages.
inline bool ntt_form_allowed(int form, uint32_t k) {
    if (form < NTT_FORM_LATENCY || form > NTT_FORM_BIG || k > NTT_MAX_LOG) return false;
    return form != NTT_FORM_MID || k >= 11;
}

struct NttLaunch {
    NttPass pass;
    uint32_t threads;     // block size
    uint32_t grid_x;      // tiles per polynomial (grid.y = the batch)
    uint32_t lds_bytes;   // dynamic LDS: the tile
};

// The launches of one chain, in the order of the global stages t0 = 0, g0, g0 + g1 ...; false for a form the size cannot take.
inline bool ntt_passes(uint32_t k, bool dif, uint32_t stride, int form, std::vector<NttLaunch>* out) {
    out->clear();
    if (!ntt_form_allowed(form, k)) return false;
    if (k == 0) return true;
    std::vector<uint32_t> gs;   // stages per pass
    uint32_t tile_log;
    if (form == NTT_FORM_MID) {
        tile_log = 11;
        const uint32_t g0 = 11, rest = k - g0, np = (rest + 8) / 9;
        std::vector<uint32_t> strided;
        for (uint32_t i = 0; i < np; i++) strided.push_back(rest / np + (i < rest % np ? 1 : 0));
        // DIF: stage t0 = 0 has the LARGEST distance, the contiguous pass comes last; DIT: first
        if (dif) {
            gs = strided;
            gs.push_back(g0);
        } else {
            gs.push_back(g0);
            gs.insert(gs.end(), strided.begin(), strided.end());
        }
    } else {
        const bool big = form == NTT_FORM_BIG;
        const uint32_t max_g = big ? zkdev::NTT_BIG_MAX_G : zkdev::NTT_MAX_G;
        tile_log = form == NTT_FORM_LATENCY ? 8 : big ? zkdev::NTT_BIG_TILE_LOG : zkdev::NTT_TILE_LOG;
        const uint32_t np = (k + max_g - 1) / max_g;
        for (uint32_t i = 0; i < np; i++) gs.push_back(k / np + (i < k % np ? 1 : 0));
    }
    uint32_t t0 = 0;
    for (uint32_t g : gs) {
        NttLaunch l;
        NttPass& p = l.pass;
        p.log_n = k;
        p.t0 = t0;
        p.g = g;
        uint32_t lcw = tile_log - p.g;
        if (lcw > k - p.g) lcw = k - p.g;
        p.log_cw = lcw;
        p.dif = dif ? 1 : 0;
        p.stride = stride;
        p.src_stride = 0;
        p.src_valid = 0;
        l.threads = form == NTT_FORM_LATENCY ? (1u << (p.g + p.log_cw - 1))
                  : form == NTT_FORM_MID     ? 512u
                  : form == NTT_FORM_BIG     ? (uint32_t)zkdev::NTT_BIG_THREADS
                                             : (uint32_t)zkdev::NTT_THREADS;
        l.grid_x = (uint32_t)((((uint64_t)1 << k) >> p.g) >> p.log_cw);
        l.lds_bytes = (1u << (p.g + p.log_cw)) * 32u;
        out->push_back(l);
        t0 += p.g;
    }
    return true;
}

}  // namespace zkrt
