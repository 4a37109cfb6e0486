"""The coefficients of the combined check of a chunk (csrc/verify_rlc.h) pinned without a GPU, through the test hook
zk_hook_rlc_coefs of the emulation build: every word the device is handed - rho_i, the scalars s_j, the exponent of
e(alpha, beta) and its bit length - against a restatement of the derivation in Python (hashlib's Blake2s, integers mod r), for
every number of host threads.

A slip in the derivation passes every verdict test: a chunk the combined check does not vouch for goes to the per-proof
verifier, and a chunk it wrongly vouches for takes a forged proof, which no test holds.  The expected values come from the
restatement below, never from the header.  The derivation never decodes a point: the proofs are random bytes, the inputs
random canonical scalars.

No draw of the fixed data below is all zero (asserted), so the replacement of a zero rho_i by 1 is covered by reading the
code only (verify_rlc.h: one line behind the memcpy of the draw); a 2^-128 event cannot be staged without a hash preimage."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001     # the order of the groups of BLS12-381
X = 0xd201000000010000                                                     # |x|, the curve parameter
LAMBDA = R - X * X
LEAF = 256
THREADS = (1, 2, 3, 7, 16)
SIZES = [(8, 3), (255, 3), (256, 3), (257, 3), (513, 1)]                   # the minimum; one leaf, one full, two; three leaves


def u64be(v):
    return v.to_bytes(8, "big")


def restated(key_digest, n, n_inputs, proofs, inputs):
    """-> (rho, s, exp, nbits) as the bytes and the number zk_hook_rlc_coefs returns"""
    seed = hashlib.blake2s(key_digest + u64be(n), person=b"zkamdrlc")
    for leaf, lo in enumerate(range(0, n, LEAF)):
        hi = min(lo + LEAF, n)
        seed.update(hashlib.blake2s(u64be(leaf) + proofs[lo * 192:hi * 192] + inputs[lo * n_inputs * 32:hi * n_inputs * 32],
                                    person=b"zkamdrlc").digest())
    seed = seed.digest()
    rho, s, sa, sb = b"", [0] * (n_inputs + 1), 0, 0
    for i in range(n):
        draw = hashlib.blake2s(seed + u64be(i)).digest()[:16]
        assert any(draw), "a zero draw in the fixed test data"
        rho += draw
        a, b = int.from_bytes(draw[:8], "little"), int.from_bytes(draw[8:], "little")
        sa, sb = sa + a, sb + b
        r = (a + b * LAMBDA) % R
        s[0] = (s[0] + r) % R
        for j in range(n_inputs):
            x = int.from_bytes(inputs[(i * n_inputs + j) * 32:(i * n_inputs + j + 1) * 32], "little")
            s[1 + j] = (s[1 + j] + r * x) % R
    exp = sa.to_bytes(16, "little") + sb.to_bytes(16, "little")
    return rho, b"".join(v.to_bytes(32, "little") for v in s), exp, max(1, sa.bit_length(), sb.bit_length())


def coefs(lib, key_digest, n, n_inputs, proofs, inputs, threads):
    fn = lib.dll.zk_hook_rlc_coefs
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p, C.c_char_p, C.c_uint, C.c_char_p, C.c_char_p, C.c_char_p,
                   C.POINTER(C.c_uint32)]
    rho, s, exp = C.create_string_buffer(16 * n), C.create_string_buffer(32 * (n_inputs + 1)), C.create_string_buffer(32)
    nbits = C.c_uint32(0)
    lib.check(fn(key_digest, n, n_inputs, proofs, inputs, threads, rho, s, exp, C.byref(nbits)))
    return rho.raw, s.raw, exp.raw, nbits.value


_cases = {}   # (n, n_inputs) -> (key_digest, proofs, inputs, restated(...)): computed once, shared by the tests, never changed


def case(n, n_inputs):
    if (n, n_inputs) not in _cases:
        rng = random.Random(1000 * n + n_inputs)
        key_digest, proofs = rng.randbytes(32), rng.randbytes(192 * n)
        inputs = b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(n * n_inputs))
        _cases[(n, n_inputs)] = (key_digest, proofs, inputs, restated(key_digest, n, n_inputs, proofs, inputs))
    return _cases[(n, n_inputs)]


def test_header_is_host_only_and_clean_under_the_sanitizers(tmp_path):
    """tests/verify_rlc_main.cpp: the header in a stand-alone program (no HIP, no library), AddressSanitizer + UBSan, 1 against
    16 threads at n = 8 and n = 257"""
    exe = str(tmp_path / "verify_rlc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(HERE, "verify_rlc_main.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and "coefficients agree" in run.stdout and not run.stderr, run.stdout + run.stderr


def test_lambda_is_a_primitive_cube_root_of_unity():
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0 and LAMBDA != 1


@pytest.mark.parametrize("n, n_inputs", SIZES)
def test_every_thread_count_gives_the_restatement(emu_lib, n, n_inputs):
    key_digest, proofs, inputs, want = case(n, n_inputs)   # (n = 8 with 16 threads: half of them get an empty range)
    for threads in THREADS:
        got = coefs(emu_lib, key_digest, n, n_inputs, proofs, inputs, threads)
        assert got == want, threads


@pytest.mark.parametrize("n, n_inputs", SIZES)
def test_bit_length_of_the_exponent(emu_lib, n, n_inputs):
    key_digest, proofs, inputs, _ = case(n, n_inputs)
    rho, _, exp, nbits = coefs(emu_lib, key_digest, n, n_inputs, proofs, inputs, 3)
    sa = sum(int.from_bytes(rho[16 * i:16 * i + 8], "little") for i in range(n))
    sb = sum(int.from_bytes(rho[16 * i + 8:16 * i + 16], "little") for i in range(n))
    assert exp == sa.to_bytes(16, "little") + sb.to_bytes(16, "little")
    assert nbits == max(1, sa.bit_length(), sb.bit_length()) and 64 < nbits <= 64 + n.bit_length()


def test_domain_separation(emu_lib):
    """the key, a proof of the second leaf, an input and the number of proofs each move the first coefficient"""
    n, n_inputs = 257, 3
    key_digest, proofs, inputs, want = case(n, n_inputs)

    def flip(b, at):
        return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]

    def rho0(*args):
        got = coefs(emu_lib, *args, 2)
        assert got == restated(*args)
        return got[0][:16]
    base = want[0][:16]
    assert rho0(key_digest, n, n_inputs, proofs, inputs) == base
    assert rho0(flip(key_digest, 31), n, n_inputs, proofs, inputs) != base
    assert rho0(key_digest, n, n_inputs, flip(proofs, 256 * 192 + 100), inputs) != base
    assert rho0(key_digest, n, n_inputs, proofs, flip(inputs, 40 * n_inputs * 32 + 5)) != base
    assert rho0(key_digest, n - 1, n_inputs, proofs[:-192], inputs[:-32 * n_inputs]) != base
