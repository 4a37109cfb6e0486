// The coefficients of the combined check (csrc/verify_rlc.h) as a stand-alone host program under AddressSanitizer and UBSan:
// the header compiles with no HIP in sight, and 1 and 16 threads give the same bytes at the minimum chunk and at two leaves
// with one proof in the second.  What the bytes must BE is tests/test_verify_rlc.py's business.
#include <stdio.h>
#include <thread>
#include <vector>
#include "../zero-chain_amd/csrc/verify_rlc.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {   // SplitMix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main() {
    auto run = [](unsigned nth, auto& work) {
        std::vector<std::thread> ths;
        for (unsigned t = 0; t < nth; t++) ths.emplace_back([&work, t] { work(t); });
        for (auto& th : ths) th.join();
    };
    const uint32_t ni = 3;
    for (size_t n : {(size_t)8, (size_t)257}) {
        std::vector<uint8_t> key(32), proofs(n * 192), inputs(n * ni * 32);
        for (auto& b : key) b = (uint8_t)next_u64();
        for (auto& b : proofs) b = (uint8_t)next_u64();
        for (size_t k = 0; k < n * ni; k++) {   // canonical: the top limb below r's
            uint64_t v[4] = {next_u64(), next_u64(), next_u64(), next_u64() >> 2};
            memcpy(&inputs[k * 32], v, 32);
        }
        const zkrlc::Coefs a = zkrlc::coefs(key.data(), n, ni, proofs.data(), inputs.data(), 1, run);
        const zkrlc::Coefs b = zkrlc::coefs(key.data(), n, ni, proofs.data(), inputs.data(), 16, run);
        if (a.rho.size() != n * 4 || a.s.size() != (ni + 1) * 8 || a.rho != b.rho || a.s != b.s || memcmp(a.exp, b.exp, 32) || a.nbits != b.nbits ||
            a.nbits < 65) {
            printf("n = %zu: 1 and 16 threads differ\n", n);
            return 1;
        }
    }
    printf("coefficients agree\n");
    return 0;
}
