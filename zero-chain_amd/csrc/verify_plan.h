// The plan of one chunk of a verification (verify.cpp): which form of every stage runs, as pure integer logic on (proofs in
// the chunk, public inputs, where the proofs come from, the tunables) - nothing here touches the HIP runtime, so the CPU
// suite pins it (tests/test_verify_plan.py, through zk_hook_verify_plan).  Every form gives the same verdicts, so a threshold
// that moves by accident passes every verdict test and only changes what a block of transfers costs.
#pragma once
#include <algorithm>
#include "host_common.h"
#include "pairing.h"
#include "coop_verify.h"

namespace zkrt {

// The combined check saves WORK (n + 2 Miller loops and one final exponentiation instead of 3 n and n), which is what a
// verification costs only once the chunk fills the machine: 1024 proofs 8.0 ms per proof against 12.7 combined, 8192: 22.5 /
// 16.0 (profiles/r05final_verify_probe.txt) - the two meet near 4000.
constexpr size_t VERIFY_RLC_AUTO_MIN = 4096;

// The environment variables a chunk reads, each with its own parsing rule.  Read once per chunk and in this one place (the
// suites flip them between calls: nothing is static).
struct VerifyTunables {
    bool wide;            // ZKAMD_VERIFY_WIDE: off only when set and atoi() of it is 0 (so an empty string is off)
    bool coop_verify;     // ZKAMD_COOP_VERIFY: 0 = no stage on rows
    bool coop_pairing;    // ZKAMD_COOP_PAIRING: 0 = the eighteen-lane pairing also where rows would take it
    bool windows;         // ZKAMD_INPUTS_WINDOWS: 0 = sixteen pieces per scalar instead of the table of 8-bit windows
    size_t inputs_max;    // ZKAMD_COOP_INPUTS_MAX: largest chunk whose input accumulator runs on rows
    size_t pairing_max;   // ZKAMD_COOP_PAIRING_MAX: largest chunk whose decoders, line preparation and pairing run on rows
    size_t fine_min;      // ZKAMD_INPUTS_FINE_MIN: smallest chunk of the large forms of the input accumulator on lanes
    size_t rlc_min;       // ZKAMD_VERIFY_RLC_MIN: smallest chunk VERIFY_AUTO hands to the combined check

    static VerifyTunables read() {
        auto env_n = [](const char* name, size_t dflt) {   // (unset or empty: the default)
            const char* e = getenv(name);
            return e && *e ? (size_t)strtoull(e, nullptr, 10) : dflt;
        };
        VerifyTunables t;
        const char* wide_env = getenv("ZKAMD_VERIFY_WIDE");
        t.wide = !(wide_env && atoi(wide_env) == 0);
        t.coop_verify = env_n("ZKAMD_COOP_VERIFY", 1) != 0;
        t.coop_pairing = env_n("ZKAMD_COOP_PAIRING", 1) != 0;
        t.windows = env_n("ZKAMD_INPUTS_WINDOWS", 1) != 0;
        t.inputs_max = env_n("ZKAMD_COOP_INPUTS_MAX", zkcoop::VERIFY_MAX);
        t.pairing_max = env_n("ZKAMD_COOP_PAIRING_MAX", zkcoop::PAIRING_MAX);
        t.fine_min = env_n("ZKAMD_INPUTS_FINE_MIN", zkdev::INPUTS_FINE_MIN);
        const char* rlc_env = getenv("ZKAMD_VERIFY_RLC_MIN");
        t.rlc_min = rlc_env ? (size_t)atoll(rlc_env) : VERIFY_RLC_AUTO_MIN;
        return t;
    }
};

// One value per lane (pairing.h) or rows of 16 lanes (coop_verify.cpp, coop_pairing.cpp): the same words between the stages
enum class VDecode { NONE, ROWS, LANES };              // NONE: the prover handed its affine coordinates over
enum class VPrepare { NONE, ROWS, TRI };               // the lines of B: NONE = the one-thread Miller loop prepares none
enum class VInputs { ROWS, WINDOWS, SIXTEEN, FOUR };   // on lanes: the table of 8-bit windows, sixteen or four pieces per scalar
enum class VPairing { ROWS, LANES18, THREAD };         // Miller loops and final exponentiation

struct VerifyPlan {
    VDecode decode;
    bool b_torsion_in_decoder;   // the lane decoder of B runs its r-torsion test itself (else the line preparation settles it)
    bool subgroup_tests;         // a foreign byte string: the decoder of A and C runs theirs, the preparation gets B's state words
    VPrepare prepare;
    size_t prep_b_points;        // points whose line tables the preparation writes to prep_b (the pairing on rows reads the stage instead)
    VInputs inputs;
    bool inputs_mul;             // the forms on lanes: a key without inputs skips the multiplication kernel and still runs the sum
    VPairing pairing;
};

// own_proofs: A, B, C were computed by this library's prover a moment ago (no r-torsion test: only a foreign byte string
// needs it); have_own_affine: ... and came with their affine coordinates (no decoding)
inline VerifyPlan verify_plan(size_t n, size_t n_inputs, bool own_proofs, bool have_own_affine, const VerifyTunables& tun) {
    // wide: eighteen lanes per (proof, pair) and per final exponentiation (pairing.h "Lane-parallel Fq12"), chains ~9x shorter
    // than one thread's, which the key's e(alpha, beta) always takes.  On rows: the input accumulator for a handful of proofs
    // (88 rows per proof: work-bound beyond inputs_max); the decoders, the line preparation of B, the Miller loops and the final
    // exponentiation (3 + 1 + 18 + 6 rows per proof) up to pairing_max proofs: shorter chains AND fewer instructions.
    const bool coop_on = tun.wide && tun.coop_verify;
    const bool coop_inputs = coop_on && n <= tun.inputs_max;
    const bool coop_head = coop_on && n <= std::max(tun.pairing_max, tun.inputs_max);
    const bool coop_pairing = coop_head && n <= tun.pairing_max && tun.coop_pairing;
    VerifyPlan p;
    p.decode = own_proofs && have_own_affine ? VDecode::NONE : coop_head ? VDecode::ROWS : VDecode::LANES;
    // (the preparation's last point settles B's r-torsion test, k_g2_prepare: the decoder leaves it out wherever lines are prepared)
    p.b_torsion_in_decoder = p.decode == VDecode::LANES && !(own_proofs || tun.wide);
    p.subgroup_tests = !own_proofs;
    p.prepare = coop_head ? VPrepare::ROWS : tun.wide ? VPrepare::TRI : VPrepare::NONE;
    p.prep_b_points = p.prepare == VPrepare::TRI || (coop_head && !coop_pairing) ? n : 0;
    p.inputs = coop_inputs                                   ? VInputs::ROWS
               : n_inputs && n >= tun.fine_min && tun.windows ? VInputs::WINDOWS   // four chains of eight additions per scalar
               : n >= tun.fine_min                            ? VInputs::SIXTEEN   // ... and a wave per proof for the sum
                                                              : VInputs::FOUR;
    p.inputs_mul = n_inputs != 0;
    p.pairing = coop_pairing ? VPairing::ROWS : tun.wide ? VPairing::LANES18 : VPairing::THREAD;
    return p;
}

// The head (decoders, line preparation) on lanes whatever the chunk's size: the reader (B's r-torsion test inside the decoder
// or at the end of the preparation, as `wide` has it) and the combined check, whose Miller loop always reads prepared lines
inline VerifyPlan verify_plan_lane_head(size_t n, bool own_proofs, VerifyTunables tun, bool force_wide) {
    tun.coop_verify = false;
    tun.wide = tun.wide || force_wide;
    return verify_plan(n, 0, own_proofs, false, tun);
}

// form: VERIFY_PER_PROOF | VERIFY_COMBINED (every chunk of 8 or more) | VERIFY_AUTO (the chunks it is the faster form for)
inline bool verify_takes_combined(int form, size_t np, const VerifyTunables& tun) {
    return (form == VERIFY_COMBINED || (form == VERIFY_AUTO && np >= tun.rlc_min)) && np >= 8;
}

}  // namespace zkrt
