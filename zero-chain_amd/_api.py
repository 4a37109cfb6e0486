"""Host-side mirror of the bellman surface LayerXcom/zero-chain consumes on its proving path,
over the C ABI of libzkamd.so (include/zkamd.h).

Reference surface being mirrored (all in the un-vendored bellman 0.1.0 crate,
called from /root/reference/core/proofs/src/confidential.rs):
    Parameters::read(reader, checked)      confidential.rs:99     -> Parameters.read
    Parameters::write(writer)              confidential.rs:83     -> Parameters.write
    create_random_proof(circuit, &pk, rng) confidential.rs:149    -> create_random_proof
    create_proof(circuit, &pk, r, s)                              -> create_proof
    Proof::write / Proof::read (192 B)     confidential.rs:294-297 -> Proof.write / Proof.read
    SynthesisError                         confidential.rs:171,272 -> ZkError.variant

The circuit itself (Circuit::synthesize + ProvingAssignment) stays on the host side of the
boundary, exactly as in the reference; what crosses it is the finished assignment
(`ProvingAssignment`: row evaluations a/b/c, input and aux assignments, density trackers).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._shard import shard_bounds, gather_proofs, prove_sharded
from ._lib import (ZkError, ZkLib, ZK_FR_MONTGOMERY, ZK_NTT_INVERSE, ZK_NTT_COSET, ZK_NTT_IN_BITREV,
                   ZK_NTT_OUT_BITREV)

__all__ = ["transfer_check", "anonymous_check", "Parameters", "Proof", "generate_parameters", "generate_random_parameters", "PreparedVerifyingKey", "prepare_verifying_key", "verify_proof", "verify_proofs", "read_proofs",
           "verify_transfer_batch", "jubjub_into_xy", "redjubjub_sign", "redjubjub_verify", "REDJUBJUB_REASONS", "verify_confidential_xts", "verify_anonymous_xts", "execute_confidential_block", "execute_anonymous_block", "execute_asset_block", "ASSET_KINDS", "BLOCK_TAKEN", "g_epoch", "BLOCK_VERDICTS", "BLOCK_ROLLOVER_DUE", "BLOCK_ROLLED", "INTO_XY_REASONS", "SCAN_SENDER", "SCAN_RECIPIENT", "CONFIDENTIAL_XT_POINTS", "ANONYMOUS_XT_POINTS", "ProvingAssignment", "create_proof", "create_random_proof", "create_proofs", "create_proofs_dev", "stream", "bind_host_to_device", "KernelTimer", "kernel_forms",
           "multiexp", "multiexp_cache_release", "memory_stats", "MultiexpContext", "ConstraintMatrices", "create_proofs_from_witness", "fs_rand", "spending_key_from_seed", "jubjub_base_mul", "jubjub_base_mul_dev", "hd_master", "hd_xpgk", "hd_derive", "HD_XKEY_BYTES", "HD_XSK", "HD_XPGK", "elgamal_encrypt", "elgamal_encrypt_dev", "ElGamalTable", "ScanKeys", "scan_confidential_keys", "scan_anonymous_keys", "balances_keys", "balance", "BALANCE_POINTS", "elgamal_add", "ledger_apply", "LEDGER_SUBTRACT", "LEDGER_SKIP", "LEDGER_SCAN_WIDTH", "balance_query", "ELGAMAL_DECRYPT_LIMIT", "ZERO_CIPHERTEXT", "transfer_requests", "transfer_derive", "gen_proofs", "xt_fields", "gen_proof", "XT_FIELDS",
           "FS_MODULUS", "transfer_statements", "transfer_witness", "transfer_witness_gpu", "transfer_r1cs_fingerprint", "anonymous_r1cs_fingerprint", "ANONYMOUS_N_INPUTS", "ANONYMOUS_N_AUX", "anonymous_statements", "anonymous_requests", "anonymous_derive", "anonymous_derive_dev", "anonymous_gen_proofs", "anonymous_witness", "anonymous_witness_gpu", "anonymous_prove_batch",
           "transfer_prove_batch", "TransferPipeline", "set_host_threads", "TRANSFER_N_INPUTS", "TRANSFER_N_AUX", "EvaluationDomain", "XorShiftRng", "fr_rand", "ZkError", "FR_MODULUS",
           "scalars_to_bytes", "bytes_to_scalars", "load_library", "ZK_FR_MONTGOMERY", "ZK_NTT_INVERSE",
           "ZK_NTT_COSET", "ZK_NTT_IN_BITREV", "ZK_NTT_OUT_BITREV", "shard_bounds", "gather_proofs", "prove_sharded"]

FR_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
_FR_R_INV = pow(1 << 256, -1, FR_MODULUS)
PROOF_SIZE = 192  # core/proofs/src/constants.rs:3


def load_library():
    return _lib.load()


def set_host_threads(n, lib=None):
    """zk_set_host_threads: host threads for the CPU-side legs (witness calculation, encoding); 0 = default."""
    (lib or _lib.load()).zk_set_host_threads(int(n))


def bind_host_to_device(device=0, lib=None):
    """zk_bind_host_to_device: pin the calling thread (and the threads it starts) to the CPUs of the GPU's NUMA node.
    Returns (numa node or -1, CPUs the thread may run on)."""
    lib = lib or _lib.load()
    node, cpus = C.c_int(-1), C.c_int(0)
    lib.check(lib.zk_bind_host_to_device(int(device), C.byref(node), C.byref(cpus)))
    return node.value, cpus.value


def kernel_forms(device=0, lib=None):
    """zk_kernel_forms: which form of the two scratch-using assembly kernels the device runs and the load-time comparison it
    was chosen by: {"g2_accumulate": 0 | 1, "reduce_level1": 0 | 1, "ms": [g2 first, g2 scratch-free, red first, red sf]}."""
    lib = lib or _lib.load()
    forms, ms = (C.c_uint32 * 2)(), (C.c_float * 4)()
    lib.check(lib.zk_kernel_forms(int(device), forms, ms))
    return {"g2_accumulate": int(forms[0]), "reduce_level1": int(forms[1]), "ms": [round(float(x), 4) for x in ms]}


class KernelTimer:
    """zk_profile_begin / zk_profile_get / zk_profile_end: HIP-event timing of the library's named kernel groups.
    with KernelTimer(lib) as t: ...;  t.get("msm_accumulate_g1") -> (launches, total ms)."""

    def __init__(self, lib=None):
        self._lib = lib or _lib.load()

    def __enter__(self):
        self._lib.zk_profile_begin()
        return self

    def get(self, name):
        ms = C.c_double(0)
        n = self._lib.zk_profile_get(name.encode(), C.byref(ms))
        return int(n), float(ms.value)

    def __exit__(self, *exc):
        self._lib.zk_profile_end()
        return False


def scalars_to_bytes(values):
    """ints in [0, 2^256) -> n x 32 bytes, plain little-endian (FrRepr::write_le).  Values are NOT
    reduced: a non-canonical scalar reaches the library and is rejected there, as in the reference
    where FrRepr -> Fr conversion fails for values >= r (fr.rs:276-289)."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def bytes_to_scalars(buf):
    b = bytes(buf)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _u8(x, n=None):
    a = np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)
    if n is not None and a.size != n:
        raise ValueError("expected %d bytes, got %d" % (n, a.size))
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ----------------------------------------------------------------------------------------------
# rand 0.4 XorShiftRng + Fr::rand, so that create_random_proof draws the same (r, s) as the
# reference for a given seed (core/pairing/src/bls12_381/fr.rs:255-267; seeds as in
# core/proofs/src/confidential.rs:511-513).
# ----------------------------------------------------------------------------------------------
class XorShiftRng:
    def __init__(self, seed):
        self.x, self.y, self.z, self.w = [int(s) & 0xFFFFFFFF for s in seed]

    @classmethod
    def from_seed(cls, seed):
        return cls(seed)

    def next_u32(self):
        t = (self.x ^ (self.x << 11)) & 0xFFFFFFFF
        self.x, self.y, self.z = self.y, self.z, self.w
        self.w = (self.w ^ (self.w >> 19) ^ (t ^ (t >> 8))) & 0xFFFFFFFF
        return self.w

    def next_u64(self):
        hi = self.next_u32()
        return (hi << 32) | self.next_u32()


def fr_rand(rng):
    """Fr::rand: 4 x next_u64 limbs, top bit shaved, rejected unless < r; the accepted limbs ARE the
    Montgomery representation.  Returns the plain integer."""
    while True:
        limbs = [rng.next_u64() for _ in range(4)]
        limbs[3] &= 0xFFFFFFFFFFFFFFFF >> 1
        v = sum(l << (64 * i) for i, l in enumerate(limbs))
        if v < FR_MODULUS:
            return v * _FR_R_INV % FR_MODULUS


# ----------------------------------------------------------------------------------------------
class Proof:
    """groth16::Proof<Bls12>: A (G1) | B (G2) | C (G1), compressed (bellman-verifier/src/lib.rs:55-65)."""

    def __init__(self, data):
        data = bytes(data)
        if len(data) != PROOF_SIZE:
            raise ValueError("a proof is exactly 192 bytes")
        self.bytes = data

    @property
    def a(self):
        return self.bytes[:48]

    @property
    def b(self):
        return self.bytes[48:144]

    @property
    def c(self):
        return self.bytes[144:]

    def write(self, writer=None):
        if writer is not None:
            writer.write(self.bytes)
        return self.bytes

    @classmethod
    def read(cls, reader):
        data = reader if isinstance(reader, (bytes, bytearray)) else reader.read(PROOF_SIZE)
        return cls(data)

    def __eq__(self, other):
        return isinstance(other, Proof) and other.bytes == self.bytes

    def __repr__(self):
        return "Proof(%s)" % self.bytes.hex()


class Parameters:
    """groth16::Parameters<Bls12>, resident on one GPU.  `read` parses bellman's Parameters::write
    format, uploads the query bases once and expands the table of all their doublings."""

    def __init__(self, lib, handle, pk_bytes):
        self._lib = lib
        self._h = handle
        self._pk = pk_bytes
        info = _lib.ParamsInfo()
        lib.check(lib.zk_params_get_info(handle, C.byref(info)))
        self.info = {f[0]: getattr(info, f[0]) for f in info._fields_}
        self.info.update(zip(("n_merged_a", "n_merged_b1", "n_merged_b2"), self.merged_bases))

    @classmethod
    def read(cls, reader, checked=True, device=0, lib=None):
        lib = lib or _lib.load()
        data = bytes(reader if isinstance(reader, (bytes, bytearray)) else reader.read())
        buf = _u8(data)
        h = C.c_void_p()
        lib.check(lib.zk_params_load(_ptr(buf), buf.size, 1 if checked else 0, device, C.byref(h)))
        return cls(lib, h, data)

    def write(self, writer=None):
        if writer is not None:
            writer.write(self._pk)
        return self._pk

    @property
    def windows(self):
        """zk_params_get_windows: the recoding widths in use - (C' jobs of a batch, A jobs, both G1 jobs of a few proofs
        made alone, the G2 job)."""
        w = (C.c_uint32 * 4)()
        self._lib.check(self._lib.zk_params_get_windows(self._h, w))
        return tuple(int(x) for x in w)

    @property
    def merged_bases(self):
        """zk_params_get_merged: entries minus distinct points of the a, b_g1 and b_g2 queries."""
        n = (C.c_uint32 * 3)()
        self._lib.check(self._lib.zk_params_get_merged(self._h, n))
        return tuple(int(x) for x in n)

    @property
    def value_pairs(self):
        """zk_params_get_pairs: {"bases": ..., "expected_merges": ...} per query (a, b_g1, b_g2, l) for the circuit the key
        was last bound to by a statement-to-proof entry; zeros before that."""
        n = (C.c_uint32 * 8)()
        self._lib.check(self._lib.zk_params_get_pairs(self._h, n))
        names = ("a", "b_g1", "b_g2", "l")
        return {"bases": dict(zip(names, (int(x) for x in n[:4]))), "expected_merges": dict(zip(names, (int(x) for x in n[4:])))}

    @property
    def vk(self):
        """The VerifyingKey section of the parameter file (uncompressed points)."""
        n_ic = self.info["n_ic"]
        b = self._pk
        return {"alpha_g1": b[0:96], "beta_g1": b[96:192], "beta_g2": b[192:384], "gamma_g2": b[384:576],
                "delta_g1": b[576:672], "delta_g2": b[672:864],
                "ic": [b[868 + 96 * i: 868 + 96 * (i + 1)] for i in range(n_ic)]}

    def close(self):
        if self._h:
            self._lib.zk_params_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


G1_GENERATOR = bytes.fromhex(
    "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
    "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
G2_GENERATOR = bytes.fromhex(
    "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
    "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be"
    "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801")


def generate_parameters(matrices, alpha, beta, gamma, delta, tau, g1=None, g2=None):
    """bellman groth16::generate_parameters for the circuit held by `matrices` (zk_generate_parameters): returns
    Parameters::write bytes.  g1 / g2 default to the standard generators (core/pairing/src/bls12_381/README.md:45-57)."""
    lib = matrices._lib
    sc = [scalars_to_bytes([int(v)]) for v in (alpha, beta, gamma, delta, tau)]
    b1, b2 = _u8(g1 or G1_GENERATOR, 96), _u8(g2 or G2_GENERATOR, 192)
    n = C.c_size_t(0)
    args = [matrices._h, _ptr(b1), _ptr(b2)] + [_ptr(x) for x in sc]
    lib.check(lib.zk_generate_parameters(*args, None, 0, C.byref(n)))     # an upper bound, no computation
    out = np.zeros(n.value, dtype=np.uint8)
    lib.check(lib.zk_generate_parameters(*args, _ptr(out), out.size, C.byref(n)))
    return out[:n.value].tobytes()


def generate_random_parameters(matrices, rng, g1=None, g2=None):
    """generate_random_parameters (core/proofs/src/setup.rs:28-31): the five trapdoor scalars alpha, beta, gamma,
    delta, tau are drawn with Fr::rand from `rng` in bellman's order.  (bellman also draws the two generators at
    random; any generators give a valid key, the standard ones are used unless g1 / g2 are given.)"""
    alpha, beta, gamma, delta, tau = (fr_rand(rng) for _ in range(5))
    return generate_parameters(matrices, alpha, beta, gamma, delta, tau, g1=g1, g2=g2)


class PreparedVerifyingKey:
    """bellman_verifier::PreparedVerifyingKey<Bls12> resident on one GPU (zk_vk): e(alpha, beta), the line
    coefficients of -gamma and -delta, the doubling tables of ic.
        PreparedVerifyingKey.read(bytes)      PreparedVerifyingKey::read  (zface/params/conf_vk.dat)
        prepare_verifying_key(params | bytes) verifier.rs:15-30
        .write()                              PreparedVerifyingKey::write"""

    def __init__(self, lib, handle):
        self._lib = lib
        self._h = handle
        n = C.c_uint32(0)
        lib.check(lib.zk_vk_num_inputs(handle, C.byref(n)))
        self.n_inputs = n.value

    @classmethod
    def read(cls, reader, device=0, lib=None):
        lib = lib or _lib.load()
        buf = _u8(bytes(reader if isinstance(reader, (bytes, bytearray)) else reader.read()))
        h = C.c_void_p()
        lib.check(lib.zk_vk_read(_ptr(buf), buf.size, device, C.byref(h)))
        return cls(lib, h)

    def write(self, writer=None):
        n = C.c_size_t(0)
        self._lib.check(self._lib.zk_vk_write(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        self._lib.check(self._lib.zk_vk_write(self._h, _ptr(out), out.size, C.byref(n)))
        data = out.tobytes()
        if writer is not None:
            writer.write(data)
        return data

    def close(self):
        if self._h:
            self._lib.zk_vk_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_verifying_key(vk, device=None, lib=None):
    """verifier.rs:15-30.  `vk`: a Parameters object (its VerifyingKey) or VerifyingKey::write bytes."""
    if isinstance(vk, Parameters):
        lib = vk._lib
        n = C.c_size_t(0)
        lib.check(lib.zk_params_write_vk(vk._h, None, 0, C.byref(n)))
        raw = np.zeros(n.value, dtype=np.uint8)
        lib.check(lib.zk_params_write_vk(vk._h, _ptr(raw), raw.size, C.byref(n)))
        device = vk.info["device"] if device is None else device
    else:
        lib = lib or _lib.load()
        raw = _u8(bytes(vk))
        device = 0 if device is None else device
    h = C.c_void_p()
    lib.check(lib.zk_vk_prepare(_ptr(raw), raw.size, device, C.byref(h)))
    return PreparedVerifyingKey(lib, h)


def verify_proofs(pvk, proofs, public_inputs, rlc=False):
    """n independent verify_proof calls on the GPU (zk_verify_batch).  proofs: list of Proof / 192-byte strings
    (or one n x 192 byte array); public_inputs: per proof the list of Fr values WITHOUT the leading ONE (or one
    n x n_inputs x 32 byte array, plain little-endian).  Returns a list of bools; raises ZkError
    MalformedVerifyingKey when the number of inputs does not fit the key (verifier.rs:38-40)."""
    if isinstance(proofs, np.ndarray):
        pb = _u8(proofs)
    else:
        pb = _u8(b"".join(p.write() if isinstance(p, Proof) else bytes(p) for p in proofs))
    if pb.size % PROOF_SIZE:
        raise ValueError("proofs: %d bytes is not a whole number of %d-byte proofs" % (pb.size, PROOF_SIZE))
    n = pb.size // PROOF_SIZE
    if isinstance(public_inputs, np.ndarray):
        ib = _u8(public_inputs)
        if n == 0:
            if ib.size:
                raise ValueError("public inputs given for zero proofs")
            n_inputs = pvk.n_inputs
        else:
            if ib.size % (32 * n):
                raise ValueError("public_inputs: %d bytes do not split into %d rows of 32-byte scalars" % (ib.size, n))
            n_inputs = ib.size // (32 * n)
    else:
        if len(public_inputs) != n:
            raise ValueError("%d proofs but %d lists of public inputs" % (n, len(public_inputs)))
        n_inputs = len(public_inputs[0]) if n else pvk.n_inputs
        if any(len(x) != n_inputs for x in public_inputs):
            raise ValueError("every proof needs the same number of public inputs")
        flat = [v for x in public_inputs for v in x]
        ib = scalars_to_bytes(flat) if flat else np.zeros(0, dtype=np.uint8)
    # the library reads exactly n * n_inputs scalars and n proofs: nothing shorter may reach it
    if ib.size != n * n_inputs * 32:
        raise ValueError("public_inputs: %d bytes, expected %d" % (ib.size, n * n_inputs * 32))
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    fn = pvk._lib.zk_verify_batch_rlc if rlc else pvk._lib.zk_verify_batch   # rlc: one combined check per chunk, per-proof on failure
    pvk._lib.check(fn(pvk._h, n, _ptr(pb) if pb.size else None, _ptr(ib) if ib.size else None, n_inputs, _ptr(ok)))
    return [bool(x) for x in ok[:n]]


def verify_proof(pvk, proof, public_inputs):
    """verifier.rs:32-63 for one proof, through the one-proof entry zk_verify_proof."""
    pb = _u8(proof.write() if isinstance(proof, Proof) else bytes(proof))
    if pb.size != PROOF_SIZE:
        raise ValueError("a proof is %d bytes" % PROOF_SIZE)
    vals = list(public_inputs)
    ib = scalars_to_bytes(vals) if vals else np.zeros(0, dtype=np.uint8)
    ok = C.c_int(0)
    pvk._lib.check(pvk._lib.zk_verify_proof(pvk._h, _ptr(pb), _ptr(ib) if ib.size else None, len(vals), C.byref(ok)))
    return bool(ok.value)


PROOF_READ_REASONS = {1: "bad encoding", 2: "not on the curve", 3: "not in the subgroup", 4: "point at infinity"}


def read_proofs(pvk, proofs):
    """zk_proof_read_batch = Proof::read (core/bellman-verifier/src/lib.rs:67-110) without the pairing: per proof None
    when every point decodes, lies in the r-torsion subgroup and is not the point at infinity, else the pair
    (point "A" | "B" | "C", reason) of the first point that fails."""
    if isinstance(proofs, np.ndarray):
        pb = _u8(proofs)
    else:
        pb = _u8(b"".join(p.write() if isinstance(p, Proof) else bytes(p) for p in proofs))
    if pb.size % PROOF_SIZE:
        raise ValueError("proofs: %d bytes is not a whole number of %d-byte proofs" % (pb.size, PROOF_SIZE))
    n = pb.size // PROOF_SIZE
    st = np.zeros(n, dtype=np.uint8)
    pvk._lib.check(pvk._lib.zk_proof_read_batch(pvk._h, n, _ptr(pb), _ptr(st)))
    return [None if not v else ("ABC"[(int(v) & 3) - 1], PROOF_READ_REASONS[int(v) >> 2]) for v in st]


def verify_transfer_batch(pvk, statements, proofs, lib=None):
    """Verify a batch of confidential-transfer proofs against the statements they were made from: the 22 public
    inputs of each statement are recomputed by the native witness calculator (the first values of its assignment).
    Returns the number of proofs that verify."""
    lib = lib or pvk._lib
    n = len(statements)
    nv = TRANSFER_N_INPUTS + TRANSFER_N_AUX
    w = transfer_witness(statements, lib=lib).reshape(n, nv * 32)
    inputs = np.ascontiguousarray(w[:, 32:TRANSFER_N_INPUTS * 32])
    return sum(verify_proofs(pvk, proofs if isinstance(proofs, np.ndarray) else list(proofs), inputs))


INTO_XY_REASONS = {1: "not in the field", 2: "not on the curve", 3: "not in the prime-order subgroup"}
# the points of an extrinsic in the reference's push order (modules/zk-system/src/lib.rs:56-165): field k is name k - 1
CONFIDENTIAL_XT_POINTS = ("enc_key_sender", "enc_key_recipient", "left_amount_sender", "left_amount_recipient", "right_randomness",
                          "left_fee", "enc_balance_left", "enc_balance_right", "rvk", "g_epoch", "nonce")
ANONYMOUS_XT_POINTS = tuple("%s[%d]" % (f, i) for f in ("enc_keys", "left_ciphertexts", "enc_balances_left", "enc_balances_right")
                            for i in range(12)) + ("right_ciphertext", "rvk", "g_epoch", "nonce")


def jubjub_into_xy(points, device=None, lib=None):
    """zk_jubjub_into_xy = IntoXY of the reference's primitives (Point::read, as_prime_order, into_xy) for a list of
    32-byte encodings (or one n x 32 byte array).  device None: the host form (device = -1); else the device whose kernel
    runs once the batch is larger than ZKAMD_INTO_XY_HOST_MAX.  Returns ([(x, y) or None], [status]): status 0, or
    1 / 2 / 3 = y not in the field / no x for that y / not in the prime-order subgroup."""
    lib = lib or _lib.load()
    pb = _u8(points) if isinstance(points, np.ndarray) else _u8(b"".join(bytes(p) for p in points))
    if pb.size % 32:
        raise ValueError("points: %d bytes is not a whole number of 32-byte encodings" % pb.size)
    n = pb.size // 32
    xy, st = np.zeros(max(n, 1) * 64, dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    lib.check(lib.zk_jubjub_into_xy(_ptr(pb) if n else None, n, -1 if device is None else int(device), _ptr(xy), _ptr(st)))
    raw = xy.tobytes()
    vals = [None if st[i] else (int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little"))
            for i in range(n)]
    return vals, [int(v) for v in st[:n]]


REDJUBJUB_REASONS = {1: "vk is not a point", 2: "Rbar is not a point", 3: "Sbar is not below the group order", 4: "the equation fails"}


def _messages(msgs):
    """(bytes of all messages, n + 1 offsets) as the two RedJubjub entries take them"""
    msgs = [bytes(m) for m in msgs]
    offs = np.zeros(len(msgs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    blob = b"".join(msgs)
    return (_u8(blob) if blob else np.zeros(1, dtype=np.uint8)), offs


def redjubjub_sign(rsks, ts, msgs, lib=None):
    """zk_redjubjub_sign = redjubjub::PrivateKey::sign for a list of keys (32-byte strings as zk_transfer_derive returns them, or
    Fs ints), the 80 random bytes T of each (the library draws none) and the messages.  Returns the 64-byte signatures."""
    lib = lib or _lib.load()
    n = len(msgs)
    if len(rsks) != n or len(ts) != n:
        raise ValueError("one key and one 80-byte T per message")
    kb = _u8(b"".join(int(k).to_bytes(32, "little") if isinstance(k, int) else bytes(k) for k in rsks), 32 * n)
    tb = _u8(b"".join(bytes(t) for t in ts), 80 * n)
    blob, offs = _messages(msgs)
    out = np.zeros(max(n, 1) * 64, dtype=np.uint8)
    lib.check(lib.zk_redjubjub_sign(n, _ptr(kb) if n else None, _ptr(tb) if n else None, _ptr(blob), _ptr(offs), _ptr(out)))
    ob = out.tobytes()
    return [ob[64 * i:64 * i + 64] for i in range(n)]


def redjubjub_verify(vks, sigs, msgs, device=None, lib=None):
    """zk_redjubjub_verify_batch = redjubjub::PublicKey::verify for every (32-byte key, 64-byte signature, message), one verdict
    each.  device None: the host form (device = -1); else the device whose kernels run once the batch is larger than
    ZKAMD_REDJUBJUB_HOST_MAX.  Returns ([accepted], [reason]): reason 0, or a key of REDJUBJUB_REASONS."""
    lib = lib or _lib.load()
    n = len(msgs)
    if len(vks) != n or len(sigs) != n:
        raise ValueError("one key and one signature per message")
    vb, sb = _u8(b"".join(bytes(v) for v in vks), 32 * n), _u8(b"".join(bytes(s) for s in sigs), 64 * n)
    blob, offs = _messages(msgs)
    ok, why = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    lib.check(lib.zk_redjubjub_verify_batch(n, _ptr(vb) if n else None, _ptr(sb) if n else None, _ptr(blob), _ptr(offs),
                                            -1 if device is None else int(device), _ptr(ok), _ptr(why)))
    return [bool(v) for v in ok[:n]], [int(v) for v in why[:n]]


def _xt_array(xts, ctype, fill):
    if isinstance(xts, C.Array) and xts._type_ is ctype:
        return xts
    arr = (ctype * len(xts))()
    for dst, x in zip(arr, xts):
        if isinstance(x, ctype):
            C.memmove(C.byref(dst), C.byref(x), C.sizeof(ctype))
        else:
            fill(dst, x)
    return arr


def _fill_confidential_xt(dst, d):
    for f in XT_FIELDS:
        getattr(dst, f)[:] = bytes(d[f])


def _fill_anonymous_xt(dst, d):
    for f in ("proof", "right_ciphertext", "nonce", "rsk", "rvk"):
        getattr(dst, f)[:] = bytes(d[f])
    for f in ("enc_keys", "left_ciphertexts"):
        for k in range(ANONYMOUS_SIZE):
            getattr(dst, f)[k][:] = bytes(d[f][k])


def _verify_xts(pvk, fn, arr, names, g_epoch, balances):
    n = len(arr)
    if isinstance(g_epoch, (bytes, bytearray)):
        ge, stride = _u8(bytes(g_epoch), 32), 0
    else:
        ge, stride = _u8(b"".join(bytes(e) for e in g_epoch), 32 * n), 32
    ok, ref = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    pvk._lib.check(fn(pvk._h, n, arr, None if balances is None else _ptr(balances), _ptr(ge) if ge.size else None, stride, _ptr(ok), _ptr(ref)))
    return ([bool(v) for v in ok[:n]],
            [None if not v else (names[(int(v) & 63) - 1], INTO_XY_REASONS[int(v) >> 6]) for v in ref[:n]])


def verify_confidential_xts(pvk, xts, g_epoch, enc_balances=None):
    """zk_confidential_verify_batch = zk_system::verify_confidential_proof (modules/zk-system/src/lib.rs:56-115) for a
    block of ConfidentialXt: the array gen_proofs(..., raw=True) returns (or a list of such structures / of the dicts of
    xt_fields).  g_epoch: one 32-byte encoding for all, or one per xt.  enc_balances: per xt the (left, right) encodings of
    the sender's stored balance; None = each xt's own enc_balance field.  Returns (verdicts, refusals): a refusal is None,
    or (field name, reason) of the first point in push order that IntoXY refuses (then the verdict is False)."""
    arr = _xt_array(xts, _lib.ConfidentialXt, _fill_confidential_xt)
    bal = None
    if enc_balances is not None:
        bal = _u8(b"".join(bytes(l) + bytes(r) for l, r in enc_balances), 64 * len(arr))
    return _verify_xts(pvk, pvk._lib.zk_confidential_verify_batch, arr, CONFIDENTIAL_XT_POINTS, g_epoch, bal)


def verify_anonymous_xts(pvk, xts, g_epoch, enc_balances):
    """zk_anonymous_verify_batch = verify_anonymous_proof (modules/zk-system/src/lib.rs:118-165) for a block of AnonymousXt:
    the dicts anonymous_gen_proofs returns (or AnonymousXt structures).  enc_balances: per xt the twelve (left, right)
    encodings of the set members' stored balances.  Returns (verdicts, refusals) as verify_confidential_xts."""
    arr = _xt_array(xts, _lib.AnonymousXt, _fill_anonymous_xt)
    if len(enc_balances) != len(arr) or any(len(b) != ANONYMOUS_SIZE for b in enc_balances):
        raise ValueError("enc_balances: %d (left, right) pairs per xt" % ANONYMOUS_SIZE)
    bal = _u8(b"".join(bytes(l) + bytes(r) for b in enc_balances for l, r in b), 64 * ANONYMOUS_SIZE * len(arr))
    return _verify_xts(pvk, pvk._lib.zk_anonymous_verify_batch, arr, ANONYMOUS_XT_POINTS, g_epoch, bal)


BLOCK_ROLLOVER_DUE, BLOCK_ROLLED = 1, 2          # flags of an account: in (last_rollover < current epoch), out (rolled over by this block)
BLOCK_VERDICTS = ("accepted", "bad signature", "nonce used", "bad account", "refused point", "invalid proof")   # ZK_BLOCK_*


def _execute_block(pvk, fn, arr, names, accounts, nonce_pool, g_epoch, sigs, msgs, asset=None):
    """asset: None, or (kinds, asset_ids, next_asset_id) for zk_asset_block_execute - the same marshalling with the asset ids
    of extrinsics and accounts beside it, and (effects, next_asset_id) between accounts_out and stats in the result"""
    lib = pvk._lib
    n, na = len(arr), len(accounts)
    acc, out = _account_array(accounts), (_lib.BlockAccount * max(na, 1))()
    pool = _u8(b"".join(bytes(x) for x in nonce_pool), 32 * len(nonce_pool)) if len(nonce_pool) else None
    sb = blob = offs = None
    if sigs is not None:
        if msgs is None or len(sigs) != n or len(msgs) != n:
            raise ValueError("one signature and one message per xt")
        sb = _u8(b"".join(bytes(s) for s in sigs), 64 * n) if n else None
        blob, offs = _messages(msgs)
    verdicts, stats, ge = (_lib.BlockVerdict * max(n, 1))(), _lib.BlockStats(), _u8(bytes(g_epoch), 32)
    head = (pvk._h, n, arr if n else None)
    signed = (None if sb is None else _ptr(sb), None if blob is None else _ptr(blob), None if offs is None else _ptr(offs))
    pooled = (len(nonce_pool), None if pool is None else _ptr(pool), _ptr(ge))
    if asset is None:
        lib.check(fn(*head, *signed, na, acc if na else None, *pooled, out if na else None, verdicts if n else None, C.byref(stats)))
    else:
        kinds, asset_ids, next_asset_id = asset
        if len(kinds) != n or len(asset_ids) != n:
            raise ValueError("one kind and one asset id per xt")
        kb = _u8(bytes(ASSET_KINDS.index(k) if isinstance(k, str) else int(k) for k in kinds), n) if n else None
        ib = np.array([int(v) for v in asset_ids], dtype=np.uint32) if n else None
        ab = np.array([int(a["asset_id"]) for a in accounts], dtype=np.uint32) if na else None
        effects, next_out = (_lib.AssetEffect * max(n, 1))(), C.c_uint32(0)
        lib.check(fn(*head, None if kb is None else _ptr(kb), None if ib is None else _ptr(ib), *signed, na, acc if na else None,
                     None if ab is None else _ptr(ab), *pooled, int(next_asset_id), out if na else None, verdicts if n else None,
                     effects if n else None, C.byref(next_out), C.byref(stats)))

    def detail(v):
        if v.verdict == 1:
            return REDJUBJUB_REASONS[v.detail]
        if v.verdict == 4:
            return (names[(v.detail & 63) - 1], INTO_XY_REASONS[v.detail >> 6])
        return None
    ct = lambda b: (bytes(b[:32]), bytes(b[32:]))
    res = ([(BLOCK_VERDICTS[v.verdict], detail(v)) for v in verdicts[:n]],
           [dict(enc_key=bytes(o.enc_key), balance=ct(o.balance), pending=ct(o.pending), flags=int(o.flags)) for o in out[:na]],
           dict(rounds=stats.rounds, proofs_verified=stats.proofs_verified, points_decoded=stats.points_decoded))
    if asset is None:
        return res
    for o, a in zip(res[1], accounts):
        o["asset_id"] = int(a["asset_id"])
    return res[:2] + ([dict(asset_id=int(fx.asset_id), first=ct(fx.first), second=ct(fx.second)) for fx in effects[:n]], int(next_out.value)) + res[2:]


def execute_confidential_block(pvk, xts, accounts, nonce_pool, g_epoch, sigs=None, msgs=None):
    """zk_confidential_block_execute = encrypted_balances::confidential_transfer (modules/encrypted-balances/src/lib.rs:25-96)
    for a block of ConfidentialXt in order (include/zkamd.h states the seven steps).  xts: as verify_confidential_xts.
    accounts: dicts with enc_key, balance and pending ((left, right) encodings; None = Ciphertext::zero()) and flags
    (BLOCK_ROLLOVER_DUE).  nonce_pool: the 32-byte nonces already used in this epoch.  sigs / msgs: the 64-byte signature and
    the signed message of every xt (the key is its rvk), or None - signatures are then not this call's business.
    Returns (verdicts, accounts_out, stats): a verdict is (name of BLOCK_VERDICTS, detail) with detail None, the reason of
    REDJUBJUB_REASONS for a bad signature, or (field name, reason) for a refused point; accounts_out are dicts like the input
    with the flags as written (BLOCK_ROLLED); stats has rounds, proofs_verified, points_decoded."""
    arr = _xt_array(xts, _lib.ConfidentialXt, _fill_confidential_xt)
    return _execute_block(pvk, pvk._lib.zk_confidential_block_execute, arr, CONFIDENTIAL_XT_POINTS, accounts, nonce_pool, g_epoch, sigs, msgs)


def execute_anonymous_block(pvk, xts, accounts, nonce_pool, g_epoch, sigs=None, msgs=None):
    """zk_anonymous_block_execute = anonymous_balances::anonymous_transfer (modules/anonymous-balances/src/lib.rs:23-82) for a
    block of AnonymousXt in order (include/zkamd.h states the seven steps).  xts: as verify_anonymous_xts; every key of a ring
    names one of `accounts`.  Arguments and result as execute_confidential_block; a refused field is named from
    ANONYMOUS_XT_POINTS, and stats["rounds"] is never more than 1: the whole block verifies in one batch."""
    arr = _xt_array(xts, _lib.AnonymousXt, _fill_anonymous_xt)
    return _execute_block(pvk, pvk._lib.zk_anonymous_block_execute, arr, ANONYMOUS_XT_POINTS, accounts, nonce_pool, g_epoch, sigs, msgs)


ASSET_KINDS = ("transfer", "issue", "destroy")   # ZK_ASSET_*
BLOCK_TAKEN = 4                                  # flag of an account, out: an accepted destroy took it in this block


def execute_asset_block(pvk, xts, kinds, asset_ids, accounts, nonce_pool, g_epoch, next_asset_id, sigs=None, msgs=None):
    """zk_asset_block_execute = encrypted_assets::issue, confidential_transfer and destroy (modules/encrypted-assets/src/lib.rs:32-83,
    :86-164, :167-215) for a block of ConfidentialXt in order (include/zkamd.h states the steps of each).  kinds: a name of
    ASSET_KINDS (or its number) per xt; asset_ids: the id a transfer or destroy names (ignored for an issue); accounts: as
    execute_confidential_block with an asset_id key - an account is keyed by (asset_id, enc_key); next_asset_id: the id the first
    accepted issue gets.  Returns (verdicts, accounts_out, effects, next_asset_id, stats): an effect is a dict with asset_id (the
    id assigned to an accepted issue, the id named by a transfer or destroy), first and second ((left, right): the ciphertext an
    accepted issue creates; the balance and the pending transfer an accepted destroy took; else zero bytes); accounts_out carry
    BLOCK_TAKEN where a destroy was accepted."""
    arr = _xt_array(xts, _lib.ConfidentialXt, _fill_confidential_xt)
    return _execute_block(pvk, pvk._lib.zk_asset_block_execute, arr, CONFIDENTIAL_XT_POINTS, accounts, nonce_pool, g_epoch, sigs, msgs,
                          asset=(kinds, asset_ids, next_asset_id))


def g_epoch(epoch, lib=None):
    """zk_g_epoch = GEpoch::group_hash (core/primitives/src/g_epoch.rs:102-110): the 32-byte g_epoch of an epoch number."""
    lib = lib or _lib.load()
    out = np.zeros(32, dtype=np.uint8)
    lib.check(lib.zk_g_epoch(int(epoch), _ptr(out)))
    return out.tobytes()


class ProvingAssignment:
    """What bellman's ProvingAssignment holds after synthesis and the per-input rows."""

    def __init__(self, a, b, c, inputs, aux, a_aux_density, b_input_density, b_aux_density, montgomery=False):
        self.a, self.b, self.c = _u8(a), _u8(b), _u8(c)
        self.inputs, self.aux = _u8(inputs), _u8(aux)
        self.n_rows = self.a.size // 32
        self.n_inputs = self.inputs.size // 32
        self.n_aux = self.aux.size // 32
        if self.b.size != self.a.size or self.c.size != self.a.size:
            raise ValueError("a, b, c must have the same length")
        self.a_aux_density = _u8(np.asarray(a_aux_density, dtype=np.uint8), self.n_aux)
        self.b_input_density = _u8(np.asarray(b_input_density, dtype=np.uint8), self.n_inputs)
        self.b_aux_density = _u8(np.asarray(b_aux_density, dtype=np.uint8), self.n_aux)
        self.flags = ZK_FR_MONTGOMERY if montgomery else 0

    @classmethod
    def from_ints(cls, a, b, c, inputs, aux, a_aux_density, b_input_density, b_aux_density):
        return cls(scalars_to_bytes(a), scalars_to_bytes(b), scalars_to_bytes(c), scalars_to_bytes(inputs),
                   scalars_to_bytes(aux), a_aux_density, b_input_density, b_aux_density)

    def _struct(self):
        s = _lib.Assignment()
        s.n_rows, s.n_inputs, s.n_aux, s.flags = self.n_rows, self.n_inputs, self.n_aux, self.flags
        for name in ("a", "b", "c", "inputs", "aux", "a_aux_density", "b_input_density", "b_aux_density"):
            setattr(s, name, getattr(self, name).ctypes.data)
        return s


def create_proof(assignment, params, r, s):
    """bellman create_proof(circuit, params, r, s) after synthesis; r, s plain integers."""
    lib = params._lib
    rb, sb = scalars_to_bytes([r]), scalars_to_bytes([s])
    out = np.zeros(PROOF_SIZE, dtype=np.uint8)
    st = assignment._struct()
    lib.check(lib.zk_prove(params._h, C.byref(st), _ptr(rb), _ptr(sb), _ptr(out)))
    return Proof(out.tobytes())


def create_random_proof(assignment, params, rng):
    """bellman create_random_proof: r = Fr::rand(rng); s = Fr::rand(rng); create_proof(.., r, s)."""
    r = fr_rand(rng)
    s = fr_rand(rng)
    return create_proof(assignment, params, r, s)


def create_proofs(assignments, params, rs):
    """Batch of independent proofs of one circuit; rs = [(r, s), ...]."""
    lib = params._lib
    n = len(assignments)
    arr = (_lib.Assignment * n)(*[a._struct() for a in assignments])
    rsb = scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(PROOF_SIZE * n, dtype=np.uint8)
    lib.check(lib.zk_prove_batch(params._h, n, arr, _ptr(rsb), _ptr(out)))
    ob = out.tobytes()
    return [Proof(ob[i * PROOF_SIZE:(i + 1) * PROOF_SIZE]) for i in range(n)]


def create_proofs_dev(params, n, n_rows, n_inputs, n_aux, d_a, d_b, d_c, d_wit, a_aux_density, b_input_density, b_aux_density, rs,
                      montgomery=False):
    """zk_prove_batch_dev: n proofs of one circuit whose assignments are already in HBM.  d_a / d_b / d_c: device pointers
    (ints) to [n][n_rows][32] bytes, d_wit to [n][n_inputs + n_aux][32]; densities: host byte arrays shared by the batch;
    rs = [(r, s), ...] on the host."""
    lib = params._lib
    da, dbi, dba = _u8(a_aux_density), _u8(b_input_density), _u8(b_aux_density)
    bt = _lib.BatchDev(n_rows, n_inputs, n_aux, ZK_FR_MONTGOMERY if montgomery else 0, d_a, d_b, d_c, d_wit, _ptr(da), _ptr(dbi), _ptr(dba))
    rsb = scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(PROOF_SIZE * max(n, 1), dtype=np.uint8)
    lib.check(lib.zk_prove_batch_dev(params._h, n, C.byref(bt), _ptr(rsb), _ptr(out)))
    ob = out.tobytes()
    return [Proof(ob[i * PROOF_SIZE:(i + 1) * PROOF_SIZE]) for i in range(n)]


class ConstraintMatrices:
    """The fixed R1CS of a circuit on the GPU (zk_r1cs): proofs are then made from the variable
    assignment alone (`create_proofs_from_witness`), the row evaluations a = A z, b = B z, c = C z
    being computed on the device.  `constraints`: list of (A, B, C), each a list of
    (variable index, coefficient) with inputs first (ONE = 0), aux variable j at n_inputs + j."""

    @classmethod
    def transfer_circuit(cls, device=0, lib=None):
        """The reference's confidential-transfer circuit, emitted natively by the library (zk_transfer_r1cs_load)."""
        self = cls.__new__(cls)
        self._lib = lib or _lib.load()
        self.n_inputs, self.n_aux = TRANSFER_N_INPUTS, TRANSFER_N_AUX
        h = C.c_void_p()
        self._lib.check(self._lib.zk_transfer_r1cs_load(device, C.byref(h)))
        self._h = h
        return self

    @classmethod
    def anonymous_circuit(cls, device=0, lib=None):
        """The reference's anonymous-transfer circuit, emitted natively by the library (zk_anonymous_r1cs_load)."""
        self = cls.__new__(cls)
        self._lib = lib or _lib.load()
        self.n_inputs, self.n_aux = ANONYMOUS_N_INPUTS, ANONYMOUS_N_AUX
        h = C.c_void_p()
        self._lib.check(self._lib.zk_anonymous_r1cs_load(device, C.byref(h)))
        self._h = h
        return self

    def __init__(self, n_inputs, n_aux, constraints, device=0, lib=None):
        self._lib = lib or _lib.load()
        self.n_inputs, self.n_aux = n_inputs, n_aux
        keep, structs = [], []
        for m in range(3):
            row_ptr, col, coeff = [0], [], []
            for con in constraints:
                for v, c in con[m]:
                    col.append(v)
                    coeff.append(int(c))
                row_ptr.append(len(col))
            rp = np.asarray(row_ptr, dtype=np.uint32)
            cl = np.asarray(col if col else [0], dtype=np.uint32)
            cf = scalars_to_bytes(coeff) if coeff else np.zeros(32, dtype=np.uint8)
            keep += [rp, cl, cf]
            st = _lib.Csr()
            st.row_ptr, st.col, st.coeff = rp.ctypes.data, cl.ctypes.data, cf.ctypes.data
            structs.append(st)
        h = C.c_void_p()
        self._lib.check(self._lib.zk_r1cs_load(n_inputs, n_aux, len(constraints), C.byref(structs[0]), C.byref(structs[1]),
                                               C.byref(structs[2]), device, C.byref(h)))
        self._h = h

    def check(self, witnesses, montgomery=False):
        """zk_r1cs_check_batch: which constraint each assignment breaks, checked on the GPU with no key.  witnesses as for
        `create_proofs_from_witness` (with montgomery=True: raw Montgomery limbs).  One (first_bad or None, n_bad, one_ok)
        per assignment: the lowest unsatisfied constraint, how many there are, and whether input 0 is ONE = 1."""
        nv = self.n_inputs + self.n_aux
        if isinstance(witnesses, np.ndarray):
            w = _u8(witnesses)
            n = w.size // (nv * 32)
            w = _u8(w, n * nv * 32)
        else:
            n = len(witnesses)
            w = scalars_to_bytes([x for z in witnesses for x in z]) if n else np.zeros(0, dtype=np.uint8)
        out = (_lib.R1csVerdict * max(n, 1))()
        self._lib.check(self._lib.zk_r1cs_check_batch(self._h, n, _ptr(w) if n else None, ZK_FR_MONTGOMERY if montgomery else 0, out))
        return _verdicts(out, n)

    def stage(self, constraint):
        """zk_r1cs_stage: (stage number or None, first constraint, count, name) of the part of a built-in circuit the
        constraint lies in; a system built from a constraint list has no table: (None, 0, n_constraints, "")."""
        stage, first, count = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        name = C.create_string_buffer(128)
        self._lib.check(self._lib.zk_r1cs_stage(self._h, constraint, C.byref(stage), C.byref(first), C.byref(count), name, len(name)))
        return (None if stage.value == 0xFFFFFFFF else stage.value), first.value, count.value, name.value.decode()

    def close(self):
        if self._h:
            self._lib.zk_r1cs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _verdicts(out, n):
    return [(None if v.first_bad == _lib.ZK_R1CS_SATISFIED else v.first_bad, v.n_bad, not (v.flags & _lib.ZK_R1CS_ONE_IS_NOT_ONE))
            for v in out[:n]]


def transfer_check(matrices, statements):
    """zk_transfer_check_batch: statements of the transfer circuit -> [(first_bad or None, n_bad, one_ok)], through the
    witness engine zk_transfer_prove_batch would pick and no key: what a prover service asks before it pays for a proof."""
    lib = matrices._lib
    n = len(statements)
    out = (_lib.R1csVerdict * max(n, 1))()
    lib.check(lib.zk_transfer_check_batch(matrices._h, n, statements, out))
    return _verdicts(out, n)


def anonymous_check(matrices, statements):
    """zk_anonymous_check_batch: the same for statements of the anonymous-transfer circuit."""
    lib = matrices._lib
    n = len(statements)
    out = (_lib.R1csVerdict * max(n, 1))()
    lib.check(lib.zk_anonymous_check_batch(matrices._h, n, statements, out))
    return _verdicts(out, n)


def create_proofs_from_witness(matrices, params, witnesses, rs, montgomery=False):
    """witnesses: list of (inputs + aux) integer lists, or an (n, n_vars * 32)-byte array."""
    lib = params._lib
    n = len(rs)
    nv = matrices.n_inputs + matrices.n_aux
    if isinstance(witnesses, np.ndarray):
        w = _u8(witnesses, n * nv * 32)
    else:
        w = scalars_to_bytes([x for z in witnesses for x in z])
    rsb = scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(PROOF_SIZE * n, dtype=np.uint8)
    lib.check(lib.zk_prove_batch_witness(params._h, matrices._h, n, _ptr(w), ZK_FR_MONTGOMERY if montgomery else 0,
                                         _ptr(rsb), _ptr(out)))
    ob = out.tobytes()
    return [Proof(ob[i * PROOF_SIZE:(i + 1) * PROOF_SIZE]) for i in range(n)]


TRANSFER_N_INPUTS, TRANSFER_N_AUX = 23, 19955


def anonymous_r1cs_fingerprint(lib=None):
    """(blake2s hex digest, n_inputs, n_aux, n_constraints) of the natively emitted anonymous-transfer circuit."""
    lib = lib or _lib.load()
    out = np.zeros(32, dtype=np.uint8)
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.check(lib.zk_anonymous_r1cs_fingerprint(_ptr(out), C.byref(a), C.byref(b), C.byref(c)))
    return out.tobytes().hex(), a.value, b.value, c.value


def transfer_r1cs_fingerprint(lib=None):
    """(blake2s hex digest, n_inputs, n_aux, n_constraints) of the natively emitted transfer circuit, the digest as
    core/proofs/src/circuit/test.rs:228-251 defines it."""
    lib = lib or _lib.load()
    out = np.zeros(32, dtype=np.uint8)
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lib.check(lib.zk_transfer_r1cs_fingerprint(_ptr(out), C.byref(a), C.byref(b), C.byref(c)))
    return out.tobytes().hex(), a.value, b.value, c.value


def transfer_statements(items):
    """items: dicts with amount, remaining_balance, fee (ints), randomness, alpha, dec_key_sender (Fs ints)
    and proof_generation_key, enc_key_recipient, enc_balance_left, enc_balance_right, g_epoch (32-byte
    Jubjub encodings) -> ctypes array of zk_transfer_statement."""
    arr = (_lib.TransferStatement * len(items))()
    for st, it in zip(arr, items):
        st.amount, st.remaining_balance, st.fee = it["amount"], it["remaining_balance"], it["fee"]
        for name in ("randomness", "alpha", "dec_key_sender"):
            getattr(st, name)[:] = int(it[name]).to_bytes(32, "little")
        for name in ("proof_generation_key", "enc_key_recipient", "enc_balance_left", "enc_balance_right", "g_epoch"):
            getattr(st, name)[:] = bytes(it[name])
    return arr


def transfer_witness(statements, montgomery=False, lib=None):
    """zk_transfer_witness: the (23 + 19955) x 32-byte variable assignment of every statement."""
    lib = lib or _lib.load()
    n = len(statements)
    out = np.zeros(n * (TRANSFER_N_INPUTS + TRANSFER_N_AUX) * 32, dtype=np.uint8)
    lib.check(lib.zk_transfer_witness(statements, n, ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
    return out


# ----------------------------------------------------------------------------------------------
# gen_proof (core/proofs/src/confidential.rs:105-172): requests -> ConfidentialXt
# ----------------------------------------------------------------------------------------------
FS_MODULUS = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
_FS_R_INV = pow(1 << 256, -1, FS_MODULUS)
XT_FIELDS = ("proof", "enc_key_sender", "enc_key_recipient", "left_amount_sender", "left_amount_recipient", "left_fee",
             "right_randomness", "rsk", "rvk", "enc_balance", "nonce")


def fs_rand(rng):
    """Fs::rand (core/jubjub/src/curve/fs.rs:255-268): 4 x next_u64 limbs, four top bits shaved, rejected unless < s;
    the accepted limbs ARE the Montgomery representation.  Returns the plain integer."""
    while True:
        limbs = [rng.next_u64() for _ in range(4)]
        limbs[3] &= 0xFFFFFFFFFFFFFFFF >> 4
        v = sum(l << (64 * i) for i, l in enumerate(limbs))
        if v < FS_MODULUS:
            return v * _FS_R_INV % FS_MODULUS


def spending_key_from_seed(seed, lib=None):
    """SpendingKey::from_seed (keys.rs:45-58)."""
    lib = lib or _lib.load()
    buf = _u8(bytes(seed))
    out = np.zeros(32, dtype=np.uint8)
    lib.check(lib.zk_spending_key_from_seed(_ptr(buf), buf.size, _ptr(out)))
    return int.from_bytes(out.tobytes(), "little")


def jubjub_base_mul(scalars, lib=None):
    """scalar * FixedGenerators::NoteCommitmentRandomness for a list of Fs scalars (zk_jubjub_base_mul;
    EncryptionKey::from_decryption_key, keys.rs:250-261).  Returns the 32-byte encodings."""
    lib = lib or _lib.load()
    sb = scalars_to_bytes(scalars)
    out = np.zeros(32 * len(scalars), dtype=np.uint8)
    lib.check(lib.zk_jubjub_base_mul(_ptr(sb) if sb.size else None, len(scalars), _ptr(out) if out.size else None))
    ob = out.tobytes()
    return [ob[i:i + 32] for i in range(0, len(ob), 32)]


def jubjub_base_mul_dev(scalars, addends=None, device=0, lib=None):
    """zk_jubjub_base_mul_dev: scalar * G, plus addends[i] (a 32-byte encoding, read without a subgroup test) where addends is
    given, always in the kernel of the key derivation on `device`.  Returns the 32-byte encodings, or with addends
    (encodings, statuses): a refused addend has its ZK_INTO_XY_* status and 32 zero bytes."""
    lib = lib or _lib.load()
    n = len(scalars)
    if addends is not None and len(addends) != n:
        raise ValueError("scalars and addends must have the same length")
    sb = scalars_to_bytes(scalars)
    ab = None if addends is None else _points(addends, n)
    out, st = np.zeros(32 * n, dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    try:
        lib.check(lib.zk_jubjub_base_mul_dev(_ptr(sb) if n else None, _ptr(ab) if ab is not None and n else None, n, int(device),
                                             _ptr(out) if n else None, _ptr(st) if ab is not None else None))
    finally:
        sb[:] = 0
    ob = out.tobytes()
    pts = [ob[i:i + 32] for i in range(0, len(ob), 32)]
    return pts if addends is None else (pts, [int(v) for v in st[:n]])


HD_XKEY_BYTES, HD_XSK, HD_XPGK = 73, 0, 1


def hd_master(seed, lib=None):
    """ExtendedSpendingKey::master (zface/src/derive/mod.rs:48-64): the 73 bytes of the master xsk of `seed` (zk_hd_master)."""
    lib = lib or _lib.load()
    buf = _u8(bytes(seed))
    out = np.zeros(HD_XKEY_BYTES, dtype=np.uint8)
    lib.check(lib.zk_hd_master(_ptr(buf) if buf.size else None, buf.size, _ptr(out)))
    return out.tobytes()


def hd_xpgk(xsk, lib=None):
    """ExtendedProofGenerationKey::from(&xsk) (mod.rs:136-146): the watch-only half of an extended spending key (zk_hd_xpgk_from_xsk)."""
    lib = lib or _lib.load()
    buf = _u8(bytes(xsk), HD_XKEY_BYTES).copy()
    out = np.zeros(HD_XKEY_BYTES, dtype=np.uint8)
    try:
        lib.check(lib.zk_hd_xpgk_from_xsk(_ptr(buf), _ptr(out)))
    finally:
        buf[:] = 0
    return out.tobytes()


def hd_derive(xkey, indices, kind=HD_XSK, device=0, want=("xkeys", "dec_keys", "enc_keys"), lib=None):
    """zk_hd_derive: the children `indices` (u32; 2^31 and above hardened) of the extended key `xkey` of `kind`.  Returns
    (xkeys, dec_keys, enc_keys): the 73-byte children of the parent's kind, the decryption keys as integers and the 32-byte
    encryption keys of their accounts; an output not named in `want` is None (and not computed)."""
    lib = lib or _lib.load()
    n = len(indices)
    buf = _u8(bytes(xkey), HD_XKEY_BYTES).copy()
    ib = np.asarray([int(i) for i in indices], dtype=np.uint32)
    outs = {"xkeys": HD_XKEY_BYTES, "dec_keys": 32, "enc_keys": 32}
    arr = {k: (np.zeros(max(w * n, 1), dtype=np.uint8) if k in want else None) for k, w in outs.items()}
    try:
        lib.check(lib.zk_hd_derive(int(kind), _ptr(buf), _ptr(ib) if n else None, n, int(device),
                                   *[_ptr(arr[k]) if arr[k] is not None else None for k in ("xkeys", "dec_keys", "enc_keys")]))
        res = []
        for k, w in outs.items():
            if arr[k] is None:
                res.append(None)
                continue
            b = arr[k].tobytes()
            rows = [b[i:i + w] for i in range(0, w * n, w)]
            res.append([int.from_bytes(r, "little") for r in rows] if k == "dec_keys" else rows)
        return tuple(res)
    finally:
        buf[:] = 0
        for a in arr.values():
            if a is not None:
                a[:] = 0


def elgamal_encrypt(values, randomness, enc_keys, lib=None):
    """elgamal::Ciphertext::encrypt (elgamal.rs:46-63) for lists of u32 values, Fs randomness and 32-byte encryption
    keys (zk_elgamal_encrypt).  Returns (left encodings, right encodings)."""
    lib = lib or _lib.load()
    n = len(values)
    if not (len(randomness) == n and len(enc_keys) == n):
        raise ValueError("values, randomness and enc_keys must have the same length")
    vb = np.asarray(values, dtype=np.uint32)
    rb = scalars_to_bytes(randomness)
    kb = _u8(b"".join(bytes(k) for k in enc_keys), 32 * n)
    left, right = np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
    if n:
        lib.check(lib.zk_elgamal_encrypt(_ptr(vb), _ptr(rb), _ptr(kb), n, _ptr(left), _ptr(right)))
    lb, rbb = left.tobytes(), right.tobytes()
    return [lb[i:i + 32] for i in range(0, 32 * n, 32)], [rbb[i:i + 32] for i in range(0, 32 * n, 32)]


def elgamal_encrypt_dev(values, randomness, enc_keys, k=1, device=0, lib=None):
    """zk_elgamal_encrypt_dev: len(randomness) groups of k keys, one Fs randomness per group - values (ints with |v| < 2^32, a
    negative one is neg_encrypt) and enc_keys (32-byte encodings) flat, group after group.  Host threads up to
    ZKAMD_ENCRYPT_HOST_MAX lefts, else two kernels on `device`.  Returns (lefts, rights, statuses): n k and n encodings, and per
    key 0 or its ZK_INTO_XY_* status - a refused key has 32 zero bytes for its left and changes nothing else."""
    lib = lib or _lib.load()
    n, k = len(randomness), int(k)
    if not (len(values) == n * k and len(enc_keys) == n * k):
        raise ValueError("values and enc_keys must hold k entries per randomness")
    vb = np.asarray([int(v) for v in values], dtype=np.int64)
    rb = scalars_to_bytes(randomness)
    kb = _u8(b"".join(bytes(e) for e in enc_keys), 32 * n * k)
    left, right, st = np.zeros(32 * n * k, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8), np.zeros(n * k, dtype=np.uint8)
    try:
        if n:
            lib.check(lib.zk_elgamal_encrypt_dev(n, k, _ptr(vb), _ptr(rb), _ptr(kb), int(device), _ptr(left), _ptr(right), _ptr(st)))
    finally:
        rb[:] = 0
    lb, rbb = left.tobytes(), right.tobytes()
    return [lb[i:i + 32] for i in range(0, 32 * n * k, 32)], [rbb[i:i + 32] for i in range(0, 32 * n, 32)], [int(s) for s in st]


ELGAMAL_DECRYPT_LIMIT = 1000000                                  # the reference's bound, elgamal.rs:100
ZERO_CIPHERTEXT = (b"\x01" + bytes(31), b"\x01" + bytes(31))     # Ciphertext::zero(): the identity twice


SCAN_SENDER, SCAN_RECIPIENT = 1, 2                                # zk_confidential_scan_result.role
SCAN_FOUND_SENT, SCAN_FOUND_FEE, SCAN_FOUND_RECEIVED = 1, 2, 4    # ... .found


def _scan_refusal(v, names):
    return None if not v else (names[(int(v) & 63) - 1], INTO_XY_REASONS[int(v) >> 6])


def _confidential_scan_dict(r):
    return {"role": r.role, "refusal": _scan_refusal(r.refusal, CONFIDENTIAL_XT_POINTS),
            "amount_sent": r.amount_sent if r.found & SCAN_FOUND_SENT else None, "fee": r.fee if r.found & SCAN_FOUND_FEE else None,
            "amount_received": r.amount_received if r.found & SCAN_FOUND_RECEIVED else None}


def _anonymous_scan_dict(r):
    return {"members": [k for k in range(ANONYMOUS_SIZE) if r.members >> k & 1], "refusal": _scan_refusal(r.refusal, ANONYMOUS_XT_POINTS),
            "delta": r.delta if r.found else None}


BALANCE_POINTS = ("balance_left", "balance_right", "pending_left", "pending_right")   # zk_balance_result.refusal: field k is name k - 1


def _balance_dict(r):
    refused = bool(r.refusal)
    return {"value": r.value if r.found else None, "enc_total": None if refused else bytes(r.enc_total), "pending_added": bool(r.pending_added),
            "refusal": _scan_refusal(r.refusal, BALANCE_POINTS)}


def _account_array(accounts):
    """zk_block_account[]: from dicts (enc_key, balance, pending as (left, right) pairs, 64 bytes or None, flags), from a packed
    array, or from its raw bytes"""
    if isinstance(accounts, C.Array) and accounts._type_ is _lib.BlockAccount:
        return accounts
    if isinstance(accounts, (bytes, bytearray, memoryview)):
        raw = bytes(accounts)
        if len(raw) % C.sizeof(_lib.BlockAccount):
            raise ValueError("%d bytes are no whole number of BlockAccount" % len(raw))
        return (_lib.BlockAccount * (len(raw) // C.sizeof(_lib.BlockAccount))).from_buffer_copy(raw)
    arr = (_lib.BlockAccount * len(accounts))()
    for dst, a in zip(arr, accounts):
        dst.enc_key[:] = bytes(a["enc_key"])
        for f in ("balance", "pending"):
            c = a.get(f) or ZERO_CIPHERTEXT
            b = bytes(c) if isinstance(c, (bytes, bytearray)) else bytes(c[0]) + bytes(c[1])
            if len(b) != 64:
                raise ValueError("a ciphertext is 64 bytes (left || right)")
            getattr(dst, f)[:] = b
        dst.flags = int(a.get("flags", 0))
    return arr


def _points(encodings, n):
    return _u8(b"".join(bytes(e) for e in encodings), 32 * n)


class ScanKeys:
    """zk_scan_keys: a set of decryption keys (Fs integers, no two equal) for ElGamalTable.scan_confidential_keys /
    scan_anonymous_keys.  The encryption key of each is derived once, here; the handle lives on the host and binds no device."""

    def __init__(self, dec_keys, lib=None):
        self._lib = lib or _lib.load()
        self._h = None
        self._n = len(dec_keys)
        kb = scalars_to_bytes([int(k) for k in dec_keys])
        h = C.c_void_p()
        try:
            self._lib.check(self._lib.zk_scan_keys_create(_ptr(kb) if kb.size else None, self._n, C.byref(h)))
        finally:
            kb[:] = 0   # (the caller's copy of the keys is the caller's)
        self._h = h

    @classmethod
    def from_hd(cls, xkey, indices, kind=HD_XSK, device=0, lib=None):
        """zk_scan_keys_create_hd: the key set of the accounts of the children `indices` of the extended key `xkey` (hd_derive's
        arguments), in index order; the encryption keys are those the derivation computed"""
        self = cls.__new__(cls)
        self._lib = lib or _lib.load()
        self._h = None
        self._n = len(indices)
        buf = _u8(bytes(xkey), HD_XKEY_BYTES).copy()
        ib = np.asarray([int(i) for i in indices], dtype=np.uint32)
        h = C.c_void_p()
        try:
            self._lib.check(self._lib.zk_scan_keys_create_hd(int(kind), _ptr(buf), _ptr(ib) if self._n else None, self._n, int(device), C.byref(h)))
        finally:
            buf[:] = 0
        self._h = h
        return self

    def __len__(self):
        return self._n

    def enc_keys(self, first=0, count=None):
        """zk_scan_keys_get: the 32-byte encryption keys of keys first .. first + count - 1 (all from `first` by default)"""
        count = max(self._n - first, 0) if count is None else count
        out = np.zeros(32 * max(count, 1), dtype=np.uint8)
        self._lib.check(self._lib.zk_scan_keys_get(self._h, int(first), int(count), _ptr(out)))
        ob = out.tobytes()
        return [ob[i:i + 32] for i in range(0, 32 * count, 32)]

    def close(self):
        if self._h:
            self._lib.zk_scan_keys_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ElGamalTable:
    """zk_elgamal_table: the baby steps { j G : j < 2^baby_bits } of the GPU discrete-log search, built once on `device` and
    kept there (baby_bits 8 .. 24, 0 = 20).  decrypt() = Ciphertext::decrypt (elgamal.rs:85-108) over [0, limit)."""

    def __init__(self, baby_bits=0, device=0, lib=None):
        self._lib = lib or _lib.load()
        h = C.c_void_p()
        self._lib.check(self._lib.zk_elgamal_table_create(int(baby_bits), int(device), C.byref(h)))
        self._h = h

    def decrypt(self, left, right, dec_keys, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_elgamal_decrypt: left / right are lists of 32-byte encodings, dec_keys one Fs integer for all or a list of one
        per ciphertext.  Returns a list of int | None (None: no x < limit with x G == left - dk right)."""
        n = len(left)
        if len(right) != n:
            raise ValueError("left and right must have the same length")
        if isinstance(dec_keys, int):
            kb, stride = scalars_to_bytes([dec_keys]), 0
        else:
            if len(dec_keys) != n:
                raise ValueError("one key for all, or one key per ciphertext")
            kb, stride = scalars_to_bytes(dec_keys), 32
        lb, rb = _points(left, n), _points(right, n)
        values, found = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        try:
            self._lib.check(self._lib.zk_elgamal_decrypt(self._h, n, _ptr(lb), _ptr(rb), _ptr(kb), stride, int(limit), _ptr(values),
                                                         _ptr(found)))
        finally:
            kb[:] = 0   # (the caller's copy of the keys is the caller's)
        return [int(v) if f else None for v, f in zip(values, found)]

    def _scan(self, fn, ctype, fill, result, xts, dec_key, limit):
        if isinstance(xts, (bytes, bytearray, memoryview)):   # the packed extrinsics as they lie in memory
            raw = bytes(xts)
            if len(raw) % C.sizeof(ctype):
                raise ValueError("%d bytes are no whole number of %s" % (len(raw), ctype.__name__))
            arr = (ctype * (len(raw) // C.sizeof(ctype))).from_buffer_copy(raw)
        else:
            arr = _xt_array(xts, ctype, fill)
        n = len(arr)
        kb = scalars_to_bytes([int(dec_key)])
        out = (result * max(n, 1))()
        try:
            self._lib.check(fn(self._h, n, arr if n else None, _ptr(kb), int(limit), out if n else None))
        finally:
            kb[:] = 0
        return out[:n]

    def scan_confidential(self, xts, dec_key, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_confidential_scan: which of the accepted ConfidentialXt `xts` - the array gen_proofs(..., raw=True) returns, a list
        of such structures or of xt_fields dicts, or their raw bytes - carry the key of `dec_key` (an Fs integer), and the amounts
        they move.  One dict per xt: role (0, SCAN_SENDER, SCAN_RECIPIENT or both), amount_sent, fee, amount_received (an int,
        or None where no value below `limit` was found or the role does not use it) and refusal (None, or (field name, reason) of
        the first used point that Ciphertext::read refuses; the values are then None).  Proofs and signatures are not looked at."""
        res = self._scan(self._lib.zk_confidential_scan, _lib.ConfidentialXt, _fill_confidential_xt, _lib.ConfidentialScanResult, xts, dec_key, limit)
        return [_confidential_scan_dict(r) for r in res]

    def scan_anonymous(self, xts, dec_key, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_anonymous_scan for accepted AnonymousXt (the dicts anonymous_gen_proofs returns, structures, or raw bytes).  One dict
        per xt: members (the positions of the key among the twelve enc_keys; empty: absent), delta (the sum over them of +amount
        received, -amount sent, 0 as a decoy; None unless every occurrence has a value with |value| < limit) and refusal."""
        res = self._scan(self._lib.zk_anonymous_scan, _lib.AnonymousXt, _fill_anonymous_xt, _lib.AnonymousScanResult, xts, dec_key, limit)
        return [_anonymous_scan_dict(r) for r in res]

    def _scan_keys(self, fn, ctype, fill, hit, per_xt, xts, keys, limit):
        """the hit array of zk_confidential_scan_keys / zk_anonymous_scan_keys, sized by the entry's own count"""
        if keys._lib is not self._lib:
            raise ValueError("the key set and the table belong to different libraries")
        if isinstance(xts, (bytes, bytearray, memoryview)):
            raw = bytes(xts)
            if len(raw) % C.sizeof(ctype):
                raise ValueError("%d bytes are no whole number of %s" % (len(raw), ctype.__name__))
            arr = (ctype * (len(raw) // C.sizeof(ctype))).from_buffer_copy(raw)
        else:
            arr = _xt_array(xts, ctype, fill)
        n = len(arr)
        cap = min(per_xt * n, 4096)   # a guess; the entry says what a fuller block needs before it starts any work
        while True:
            out, count = (hit * max(cap, 1))(), C.c_size_t(0)
            rc = fn(self._h, keys._h, n, arr if n else None, int(limit), out, cap, C.byref(count))
            if rc != 0 and count.value > cap:
                cap = count.value
                continue
            self._lib.check(rc)
            return out[:count.value]

    def scan_confidential_keys(self, xts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_confidential_scan_keys: `xts` as scan_confidential takes them, read with every key of the ScanKeys `keys` in one
        call.  Returns [(xt, key, dict)] in (xt, key) order: one entry per extrinsic and key of the set that it carries, the dict
        being scan_confidential's for that key (a transfer between two keys of the set appears twice, one to oneself once with
        role 3)."""
        res = self._scan_keys(self._lib.zk_confidential_scan_keys, _lib.ConfidentialXt, _fill_confidential_xt, _lib.ConfidentialScanHit, 2, xts, keys, limit)
        return [(h.xt, h.key, _confidential_scan_dict(h.r)) for h in res]

    def scan_anonymous_keys(self, xts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_anonymous_scan_keys: [(xt, key, dict)] in (xt, key) order, the dict being scan_anonymous's for that key; a ring can
        appear up to twelve times."""
        res = self._scan_keys(self._lib.zk_anonymous_scan_keys, _lib.AnonymousXt, _fill_anonymous_xt, _lib.AnonymousScanHit, ANONYMOUS_SIZE, xts, keys, limit)
        return [(h.xt, h.key, _anonymous_scan_dict(h.r)) for h in res]

    def balances(self, accounts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
        """zk_balance_keys = BalanceQuery::get_balance_from_decryption_key (zface/src/utils/getter.rs:135-175) for every account
        that a key of the ScanKeys `keys` owns, in one call.  accounts: dicts as execute_confidential_block takes and returns
        them (enc_key, balance, pending, flags; its accounts_out can be passed straight in), an array of _lib.BlockAccount, or
        its raw bytes.  An account with BLOCK_ROLLOVER_DUE in its flags is read as balance + pending - set the bit everywhere
        for the reference's getter - any other as balance alone.  Returns [(account, key, dict)] in account order: value (an
        int, or None where no value below `limit` was found), enc_total (the 64 bytes left | right a transfer request carries as
        its encrypted balance), pending_added, and refusal (None, or (name of BALANCE_POINTS, reason) of the first used point
        that Ciphertext::read refuses; value and enc_total are then None)."""
        if keys._lib is not self._lib:
            raise ValueError("the key set and the table belong to different libraries")
        arr = _account_array(accounts)
        n = len(arr)
        cap = n   # (every account a hit at the most)
        out, count = (_lib.BalanceHit * max(cap, 1))(), C.c_size_t(0)
        self._lib.check(self._lib.zk_balance_keys(self._h, keys._h, n, arr if n else None, int(limit), out, cap, C.byref(count)))
        return [(h.account, h.key, _balance_dict(h.r)) for h in out[:count.value]]

    def close(self):
        if self._h:
            self._lib.zk_elgamal_table_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scan_confidential_keys(table, xts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
    """ElGamalTable.scan_confidential_keys of `table`"""
    return table.scan_confidential_keys(xts, keys, limit)


def scan_anonymous_keys(table, xts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
    """ElGamalTable.scan_anonymous_keys of `table`"""
    return table.scan_anonymous_keys(xts, keys, limit)


def balances_keys(table, accounts, keys, limit=ELGAMAL_DECRYPT_LIMIT):
    """ElGamalTable.balances of `table`"""
    return table.balances(accounts, keys, limit)


def balance(table, account, dec_key, limit=ELGAMAL_DECRYPT_LIMIT):
    """zk_balance_keys for ONE account and the key that owns it (an Fs integer): the dict of ElGamalTable.balances.  A dec_key
    whose encryption key is not the account's enc_key is a ValueError."""
    with ScanKeys([int(dec_key)], lib=table._lib) as keys:
        res = table.balances([account], keys, limit)
    if not res:
        raise ValueError("the account does not belong to this decryption key")
    return res[0][2]


def elgamal_add(left_a, right_a, left_b, right_b, subtract=False, lib=None):
    """zk_elgamal_add: Ciphertext::add (or ::sub, subtract=True; elgamal.rs:139-158) of lists of 32-byte encodings.
    Returns (left encodings, right encodings)."""
    lib = lib or _lib.load()
    n = len(left_a)
    if not (len(right_a) == len(left_b) == len(right_b) == n):
        raise ValueError("the four lists must have the same length")
    ins = [_points(x, n) for x in (left_a, right_a, left_b, right_b)]
    left, right = np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
    if n:
        lib.check(lib.zk_elgamal_add(*[_ptr(a) for a in ins], n, 1 if subtract else 0, _ptr(left), _ptr(right)))
    lb, rbb = left.tobytes(), right.tobytes()
    return [lb[i:i + 32] for i in range(0, 32 * n, 32)], [rbb[i:i + 32] for i in range(0, 32 * n, 32)]


LEDGER_SUBTRACT, LEDGER_SKIP = 1, 2   # zk_ledger_op.flags
LEDGER_SCAN_WIDTH = 256                # lanes of a workgroup of the device form's scan (csrc/ledger.h LEDGER_SCAN_W)


def _ciphertext_refusal(v):
    return None if not v else (("left", "right")[(int(v) & 63) - 1], INTO_XY_REASONS[int(v) >> 6])


def ledger_apply(slots, ops, device=None, want_before=True, lib=None):
    """zk_elgamal_ledger_apply: a block's rollover / sub_enc_balance / add_pending_transfer (the reference's three balance
    modules) - Ciphertext::add / ::sub applied to stored ciphertexts one op after another.  slots: (left, right) pairs of
    32-byte encodings, or 64-byte strings.  ops: (slot, flags, left, right) tuples - flags LEDGER_SUBTRACT | LEDGER_SKIP - or
    an array of _lib.LedgerOp.  device None: the host form (device = -1); else the device whose kernels run once the call
    holds more than ZKAMD_INTO_XY_HOST_MAX points.  Returns (slots_out, before, slot_refusals, op_refusals): 64-byte values
    (bytes(64) for a refused slot and for the ops on it), `before` None without want_before, and a refusal None or (field,
    reason) of the first point refused, field "left" or "right"."""
    lib = lib or _lib.load()

    def pair(c):
        b = bytes(c) if isinstance(c, (bytes, bytearray)) else bytes(c[0]) + bytes(c[1])
        if len(b) != 64:
            raise ValueError("a ciphertext is 64 bytes (left || right)")
        return b
    ns = len(slots)
    sb = _u8(b"".join(pair(c) for c in slots), 64 * ns)
    if isinstance(ops, C.Array) and ops._type_ is _lib.LedgerOp:
        arr = ops
    else:
        arr = (_lib.LedgerOp * len(ops))()
        for dst, (slot, flags, left, right) in zip(arr, ops):
            dst.slot, dst.flags = int(slot), int(flags)
            dst.left[:], dst.right[:] = bytes(left), bytes(right)
    no = len(arr)
    so, bo = np.zeros(max(ns, 1) * 64, dtype=np.uint8), np.zeros(max(no, 1) * 64, dtype=np.uint8)
    ss, os_ = np.zeros(max(ns, 1), dtype=np.uint8), np.zeros(max(no, 1), dtype=np.uint8)
    lib.check(lib.zk_elgamal_ledger_apply(ns, _ptr(sb) if ns else None, no, arr if no else None, -1 if device is None else int(device), _ptr(so),
                                          _ptr(bo) if want_before else None, _ptr(ss), _ptr(os_)))
    sob, bob = so.tobytes(), bo.tobytes()
    return ([sob[64 * i:64 * i + 64] for i in range(ns)], [bob[64 * i:64 * i + 64] for i in range(no)] if want_before else None,
            [_ciphertext_refusal(v) for v in ss[:ns]], [_ciphertext_refusal(v) for v in os_[:no]])


def balance_query(dec_key, encrypted_balance=None, pending_transfer=None, table=None, limit=ELGAMAL_DECRYPT_LIMIT):
    """BalanceQuery::get_balance_from_decryption_key (zface/src/utils/getter.rs:135-174): the encrypted balance plus the
    pending transfer (each 64 bytes left || right, or a (left, right) pair; an absent part is Ciphertext::zero()), decrypted
    with dec_key.  Returns (value or None, enc_total): the 64 bytes enc_total are what a transfer request carries as
    enc_balance_left || enc_balance_right.  table: an ElGamalTable to search with (default: a fresh one of 20 bits)."""
    def parts(c):
        if c is None:
            return ZERO_CIPHERTEXT
        b = bytes(c) if isinstance(c, (bytes, bytearray)) else bytes(c[0]) + bytes(c[1])
        if len(b) != 64:
            raise ValueError("a ciphertext is 64 bytes (left || right)")
        return b[:32], b[32:]
    lib = table._lib if table is not None else _lib.load()
    a, b = parts(encrypted_balance), parts(pending_transfer)
    (left,), (right,) = elgamal_add([a[0]], [a[1]], [b[0]], [b[1]], lib=lib)
    t = table if table is not None else ElGamalTable(lib=lib)
    try:
        value = t.decrypt([left], [right], int(dec_key), limit=limit)[0]
    finally:
        if table is None:
            t.close()
    return value, left + right


def transfer_requests(items):
    """items: dicts with amount, fee, remaining_balance (ints), spending_key, randomness, alpha (Fs ints) and
    enc_key_recipient, enc_balance_left, enc_balance_right, g_epoch (32-byte Jubjub encodings)."""
    arr = (_lib.TransferRequest * len(items))()
    for rq, it in zip(arr, items):
        rq.amount, rq.fee, rq.remaining_balance = it["amount"], it["fee"], it["remaining_balance"]
        for name in ("spending_key", "randomness", "alpha"):
            getattr(rq, name)[:] = int(it[name]).to_bytes(32, "little")
        for name in ("enc_key_recipient", "enc_balance_left", "enc_balance_right", "g_epoch"):
            getattr(rq, name)[:] = bytes(it[name])
    return arr


def transfer_derive(requests, lib=None):
    """zk_transfer_derive: (statements, [rsk bytes]) - the host half of gen_proof."""
    lib = lib or _lib.load()
    n = len(requests)
    st = (_lib.TransferStatement * n)()
    rsk = np.zeros(32 * n, dtype=np.uint8)
    lib.check(lib.zk_transfer_derive(requests, n, st, _ptr(rsk)))
    return st, [rsk[32 * i:32 * i + 32].tobytes() for i in range(n)]


def gen_proofs(params, matrices, pvk, requests, rs, raw=False):
    """zk_transfer_gen_proof_batch: one ConfidentialXt (dict of byte strings, XT_FIELDS) per request; raises ZkError
    Unsatisfiable when a proof fails the self-check, as the reference's gen_proof.  raw=True: the array of
    ConfidentialXt structures as the library filled it (xt_fields() turns one into the dict)."""
    lib = params._lib
    n = len(requests)
    rsb = rs if isinstance(rs, np.ndarray) else scalars_to_bytes([x for pair in rs for x in pair])
    out = (_lib.ConfidentialXt * n)()
    lib.check(lib.zk_transfer_gen_proof_batch(params._h, matrices._h, pvk._h, n, requests, _ptr(rsb), out))
    return out if raw else [xt_fields(x) for x in out]


def xt_fields(x):
    return {f: bytes(getattr(x, f)) for f in XT_FIELDS}


def gen_proof(params, matrices, pvk, amount, fee, remaining_balance, spending_key, enc_key_recipient, encrypted_balance, g_epoch, rng):
    """ProofBuilder::gen_proof for one transfer, drawing from `rng` in the reference's order: randomness and alpha
    (Fs::rand), then r and s of create_random_proof (Fr::rand)."""
    randomness, alpha = fs_rand(rng), fs_rand(rng)
    r, s = fr_rand(rng), fr_rand(rng)
    rq = transfer_requests([dict(amount=amount, fee=fee, remaining_balance=remaining_balance, spending_key=spending_key,
                                 enc_key_recipient=enc_key_recipient, enc_balance_left=encrypted_balance[0],
                                 enc_balance_right=encrypted_balance[1], g_epoch=g_epoch, randomness=randomness, alpha=alpha)])
    return gen_proofs(params, matrices, pvk, rq, [(r, s)])[0]


def transfer_witness_gpu(matrices, statements, montgomery=False):
    """zk_transfer_witness_gpu: the assignments the GPU witness generator produces (same format as transfer_witness)."""
    lib = matrices._lib
    n = len(statements)
    out = np.zeros(n * (TRANSFER_N_INPUTS + TRANSFER_N_AUX) * 32, dtype=np.uint8)
    lib.check(lib.zk_transfer_witness_gpu(matrices._h, statements, n, ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
    return out


ANONYMOUS_SIZE, ANONYMOUS_N_INPUTS, ANONYMOUS_N_AUX = 12, 105, 50429


def anonymous_statements(items):
    """items: dicts with amount, remaining_balance, s_index, t_index (ints), randomness, alpha, dec_key (Fs
    ints), proof_generation_key, g_epoch (32-byte Jubjub encodings) and enc_keys, left_ciphertexts,
    enc_balances_left, enc_balances_right (12 encodings each) -> ctypes array of zk_anonymous_statement."""
    arr = (_lib.AnonymousStatement * len(items))()
    for st, it in zip(arr, items):
        st.amount, st.remaining_balance, st.s_index, st.t_index = it["amount"], it["remaining_balance"], it["s_index"], it["t_index"]
        for name in ("randomness", "alpha", "dec_key"):
            getattr(st, name)[:] = int(it[name]).to_bytes(32, "little")
        for name in ("proof_generation_key", "g_epoch"):
            getattr(st, name)[:] = bytes(it[name])
        for name in ("enc_keys", "left_ciphertexts", "enc_balances_left", "enc_balances_right"):
            if len(it[name]) != ANONYMOUS_SIZE:
                raise ValueError("%s: expected %d members" % (name, ANONYMOUS_SIZE))
            for k, enc in enumerate(it[name]):
                getattr(st, name)[k][:] = bytes(enc)
    return arr


def anonymous_witness(statements, montgomery=False, lib=None):
    """zk_anonymous_witness: the (105 + 50429) x 32-byte variable assignment of every statement."""
    lib = lib or _lib.load()
    n = len(statements)
    out = np.zeros(n * (ANONYMOUS_N_INPUTS + ANONYMOUS_N_AUX) * 32, dtype=np.uint8)
    lib.check(lib.zk_anonymous_witness(statements, n, ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
    return out


def anonymous_witness_gpu(matrices, statements, montgomery=False):
    """zk_anonymous_witness_gpu: the assignments the GPU witness generator produces (same format as anonymous_witness)."""
    lib = matrices._lib
    n = len(statements)
    out = np.zeros(n * (ANONYMOUS_N_INPUTS + ANONYMOUS_N_AUX) * 32, dtype=np.uint8)
    lib.check(lib.zk_anonymous_witness_gpu(matrices._h, statements, n, ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
    return out


def anonymous_prove_batch(matrices, params, statements, rs):
    """zk_anonymous_prove_batch: statements of the anonymous-transfer circuit -> proofs."""
    lib = params._lib
    n = len(statements)
    rsb = scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(PROOF_SIZE * n, dtype=np.uint8)
    lib.check(lib.zk_anonymous_prove_batch(params._h, matrices._h, n, statements, _ptr(rsb), _ptr(out)))
    ob = out.tobytes()
    return [Proof(ob[i * PROOF_SIZE:(i + 1) * PROOF_SIZE]) for i in range(n)]


def anonymous_requests(items):
    """items: dicts with amount, remaining_balance, s_index, t_index (ints), spending_key, randomness, alpha (Fs ints),
    enc_key_recipient, g_epoch (32-byte Jubjub encodings), enc_keys_decoy (10 encodings) and enc_balances_left /
    enc_balances_right (12 encodings each, by set member)."""
    arr = (_lib.AnonymousRequest * len(items))()
    for rq, it in zip(arr, items):
        rq.amount, rq.remaining_balance, rq.s_index, rq.t_index = it["amount"], it["remaining_balance"], it["s_index"], it["t_index"]
        for name in ("spending_key", "randomness", "alpha"):
            getattr(rq, name)[:] = int(it[name]).to_bytes(32, "little")
        for name in ("enc_key_recipient", "g_epoch"):
            getattr(rq, name)[:] = bytes(it[name])
        for name, count in (("enc_keys_decoy", ANONYMOUS_SIZE - 2), ("enc_balances_left", ANONYMOUS_SIZE), ("enc_balances_right", ANONYMOUS_SIZE)):
            if len(it[name]) != count:
                raise ValueError("%s: expected %d encodings" % (name, count))
            for k in range(count):
                getattr(rq, name)[k][:] = bytes(it[name][k])
    return arr


def anonymous_derive(requests, lib=None):
    """zk_anonymous_derive: (statements, [rsk bytes]) - the host half of the anonymous gen_proof."""
    lib = lib or _lib.load()
    n = len(requests)
    st = (_lib.AnonymousStatement * n)()
    rsk = np.zeros(32 * n, dtype=np.uint8)
    lib.check(lib.zk_anonymous_derive(requests, n, st, _ptr(rsk)))
    return st, [rsk[32 * i:32 * i + 32].tobytes() for i in range(n)]


def anonymous_derive_dev(requests, device=0, want_inputs=False, lib=None):
    """zk_anonymous_derive_dev: (statements, [rsk bytes]) as anonymous_derive's, the point work in two kernels on `device` above
    ZKAMD_ANON_DERIVE_HOST_MAX requests; with want_inputs also the public inputs of check_proof, 104 Fr ints per request, in the
    order verify_proofs takes them for this circuit."""
    lib = lib or _lib.load()
    n = len(requests)
    st = (_lib.AnonymousStatement * n)()
    rsk = np.zeros(32 * n, dtype=np.uint8)
    inputs = np.zeros(104 * 32 * n, dtype=np.uint8) if want_inputs else None
    lib.check(lib.zk_anonymous_derive_dev(requests, n, int(device), st, _ptr(rsk), _ptr(inputs) if want_inputs else None))
    rsks = [rsk[32 * i:32 * i + 32].tobytes() for i in range(n)]
    if not want_inputs:
        return st, rsks
    flat = bytes_to_scalars(inputs)
    return st, rsks, [flat[104 * i:104 * (i + 1)] for i in range(n)]


def anonymous_gen_proofs(params, matrices, pvk, requests, rs):
    """zk_anonymous_gen_proof_batch: one AnonymousXt per request, as a dict of byte strings (enc_keys and
    left_ciphertexts: lists of 12); raises ZkError Unsatisfiable when a proof fails the self-check."""
    lib = params._lib
    n = len(requests)
    rsb = rs if isinstance(rs, np.ndarray) else scalars_to_bytes([x for pair in rs for x in pair])
    out = (_lib.AnonymousXt * n)()
    lib.check(lib.zk_anonymous_gen_proof_batch(params._h, matrices._h, pvk._h, n, requests, _ptr(rsb), out))
    res = []
    for x in out:
        d = {f: bytes(getattr(x, f)) for f in ("proof", "right_ciphertext", "nonce", "rsk", "rvk")}
        d["enc_keys"] = [bytes(e) for e in x.enc_keys]
        d["left_ciphertexts"] = [bytes(e) for e in x.left_ciphertexts]
        res.append(d)
    return res


def transfer_prove_batch(matrices, params, statements, rs):
    """zk_transfer_prove_batch: statements -> witnesses (the GPU generator; the native host calculator for a handful of
    statements, ZKAMD_WITNESS = gpu | host forces one) -> row evaluations + create_proof (GPU)."""
    lib = params._lib
    n = len(statements)
    rsb = scalars_to_bytes([x for pair in rs for x in pair])
    out = np.zeros(PROOF_SIZE * n, dtype=np.uint8)
    lib.check(lib.zk_transfer_prove_batch(params._h, matrices._h, n, statements, _ptr(rsb), _ptr(out)))
    ob = out.tobytes()
    return [Proof(ob[i * PROOF_SIZE:(i + 1) * PROOF_SIZE]) for i in range(n)]


class TransferPipeline:
    """zk_pipeline: a stream of statement batches; the witness kernels of batch k + 1 run beside the proving of
    batch k, two batches in flight on two lanes (ZKAMD_WITNESS=host: the host calculator on the host cores instead).
    submit() returns at once, wait() returns the proofs of everything submitted
    since the last wait, in submission order."""

    def __init__(self, matrices, params):
        self._lib = params._lib
        self._keep = (matrices, params)
        h = C.c_void_p()
        self._lib.check(self._lib.zk_pipeline_create(params._h, matrices._h, C.byref(h)))
        self._h = h
        self._pending = []

    @property
    def lanes(self):
        """chunks proved concurrently (zk_pipeline_lanes)"""
        return int(self._lib.zk_pipeline_lanes(self._h))

    def submit(self, statements, rs):
        n = len(statements)
        rsb = rs if isinstance(rs, np.ndarray) else scalars_to_bytes([x for pair in rs for x in pair])
        out = np.zeros(PROOF_SIZE * n, dtype=np.uint8)
        self._pending.append((statements, rsb, out))   # the buffers stay alive until wait()
        self._lib.check(self._lib.zk_pipeline_submit(self._h, n, statements, _ptr(rsb), _ptr(out)))
        return out

    def wait(self, raw=False):
        try:
            self._lib.check(self._lib.zk_pipeline_wait(self._h))
            if raw:
                return [out for _, _, out in self._pending]
            proofs = []
            for _, _, out in self._pending:
                ob = out.tobytes()
                proofs += [Proof(ob[i:i + PROOF_SIZE]) for i in range(0, len(ob), PROOF_SIZE)]
            return proofs
        finally:
            self._pending = []

    def close(self):
        if self._h:
            self._lib.zk_pipeline_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------
class MultiexpContext:
    """Bases resident on the GPU (window tables built once); run() = bellman multiexp, FullDensity."""

    def __init__(self, group, bases, window_bits=0, checked=False, device=0, lib=None, variable_base=False):
        """variable_base=True: no table of doublings (zk_msm_create_variable): classic Pippenger over the bases."""
        self._lib = lib or _lib.load()
        self.group = {"g1": 1, "g2": 2, 1: 1, 2: 2}[group]
        self.point_size = 96 if self.group == 1 else 192
        b = _u8(bases)
        self.n = b.size // self.point_size
        h = C.c_void_p()
        create = self._lib.zk_msm_create_variable if variable_base else self._lib.zk_msm_create
        self._lib.check(create(self.group, _ptr(b), self.n, window_bits, 1 if checked else 0, device, C.byref(h)))
        self._h = h

    def run(self, scalars, montgomery=False):
        s = _u8(scalars, self.n * 32) if not isinstance(scalars, (list, tuple)) else scalars_to_bytes(scalars)
        out = np.zeros(self.point_size, dtype=np.uint8)
        self._lib.check(self._lib.zk_msm_run(self._h, _ptr(s), ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
        return out.tobytes()

    def run_dev(self, d_scalars_ptr, montgomery=False):
        out = np.zeros(self.point_size, dtype=np.uint8)
        self._lib.check(self._lib.zk_msm_run_dev(self._h, C.c_void_p(d_scalars_ptr),
                                                 ZK_FR_MONTGOMERY if montgomery else 0, _ptr(out)))
        return out.tobytes()

    def close(self):
        if self._h:
            self._lib.zk_msm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multiexp_cache_release(lib=None):
    """zk_msm_cache_release: drop the handles the one-shot entries keep per (device, group)."""
    (lib or load_library()).zk_msm_cache_release()


def memory_stats(lib=None):
    """zk_memory_stats as a dict: bytes held on the device / page-locked, released so far, zeroed before release."""
    out = (C.c_uint64 * 6)()
    (lib or load_library()).zk_memory_stats(out)
    return dict(zip(("device_held", "device_released", "device_wiped", "pinned_held", "pinned_released", "pinned_wiped"), [int(v) for v in out]))


def multiexp(group, bases, scalars, lib=None):
    """bellman multiexp(FullDensity) called once: the one-shot entries zk_msm_g1 / zk_msm_g2 (variable-base Pippenger over
    fresh bases, the encodings decoded on the device, no table of doublings).  bases: n x 96 / 192 bytes uncompressed;
    scalars: ints or n x 32 bytes plain little-endian; returns the uncompressed result."""
    lib = lib or load_library()
    if group not in (1, 2):
        raise ValueError("group must be 1 (G1) or 2 (G2)")
    size = 96 if group == 1 else 192
    bb = _u8(bases)
    if bb.size % size:
        raise ValueError("bases: %d bytes is not a whole number of %d-byte points" % (bb.size, size))
    n = bb.size // size
    sb = _u8(scalars) if isinstance(scalars, (np.ndarray, bytes, bytearray)) else (scalars_to_bytes(scalars) if len(scalars) else np.zeros(0, dtype=np.uint8))
    if sb.size != 32 * n:
        raise ValueError("%d bases but %d bytes of scalars" % (n, sb.size))
    out = np.zeros(size, dtype=np.uint8)
    fn = lib.zk_msm_g1 if group == 1 else lib.zk_msm_g2
    lib.check(fn(_ptr(bb) if n else None, _ptr(sb) if n else None, n, _ptr(out)))
    return out.tobytes()


def stream(lib=None):
    """The hipStream_t (as an integer) the library enqueues its work on for the calling thread (zk_stream): what a caller
    records events on, or makes its own streams wait for, when it feeds zk_*_dev entries from its own kernels."""
    lib = lib or load_library()
    return lib.zk_stream() or 0


class EvaluationDomain:
    """bellman EvaluationDomain over Fr: fft / ifft / coset_fft / icoset_fft on lists of ints."""

    def __init__(self, coeffs, lib=None):
        self._lib = lib or _lib.load()
        n = len(coeffs)
        m, exp = 1, 0
        while m < n:
            m *= 2
            exp += 1
        self.exp = exp
        self.coeffs = [int(c) for c in coeffs] + [0] * (m - n)

    def _run(self, inverse, coset):
        buf = scalars_to_bytes(self.coeffs)
        self._lib.check(self._lib.zk_ntt_fr(_ptr(buf), self.exp, inverse, coset))
        self.coeffs = bytes_to_scalars(buf)

    def fft(self):
        self._run(0, 0)

    def ifft(self):
        self._run(1, 0)

    def coset_fft(self):
        self._run(0, 1)

    def icoset_fft(self):
        self._run(1, 1)

    def into_coeffs(self):
        return list(self.coeffs)
