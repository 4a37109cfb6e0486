// The CPU baseline of tools/decrypt_probe.py: the decryption loop of the reference (core/proofs/src/no_std_aliases/
// elgamal.rs:92-107) restated on one core over the library's host Jubjub arithmetic (csrc/transfer_witness.h): acc = O, then
// up to 10^6 times "acc == v ? i : acc += G", in extended coordinates with the projective equality test.
// Build: c++ -O2 -std=c++17 tools/ubench/elgamal_walk.cpp -o elgamal_walk;  run: elgamal_walk [value]  -> one JSON line.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "../../zero-chain_amd/csrc/transfer_witness.h"

int main(int argc, char** argv) {
    const uint64_t value = argc > 1 ? strtoull(argv[1], nullptr, 10) : 999999;
    const zkwit::EPoint g = zkwit::to_ext(zkwit::tables().win[0][1]);
    zkwit::EPoint v = zkwit::ext_zero();   // v = value G: the point a decryption ends with
    for (int bit = 63; bit >= 0; bit--) {
        v = zkwit::ext_add(v, v);
        if ((value >> bit) & 1) v = zkwit::ext_add(v, g);
    }
    const auto t0 = std::chrono::steady_clock::now();
    zkwit::EPoint acc = zkwit::ext_zero();
    long found = -1, steps = 0;
    for (long i = 0; i < 1000000; i++, steps++) {
        if (acc.X * v.Z == v.X * acc.Z && acc.Y * v.Z == v.Y * acc.Z) {
            found = i;
            break;
        }
        acc = zkwit::ext_add(acc, g);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"value\": %llu, \"found\": %ld, \"steps\": %ld, \"ms\": %.3f, \"ns_per_step\": %.1f}\n", (unsigned long long)value, found,
           steps, ms, steps ? ms * 1e6 / steps : 0.0);
    return found == (long)value || (value >= 1000000 && found < 0) ? 0 : 1;
}
