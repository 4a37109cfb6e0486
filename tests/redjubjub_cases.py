"""RedJubjub (zk_redjubjub_sign, zk_redjubjub_verify_batch) against a restatement of the reference over oracle/jubjub.py, and
the pool of signatures the tests of tests/test_redjubjub.py share.  Every function takes `lib` (a ZkLib over one build of the C
ABI); `device` None = the host form."""
import ctypes as C
import functools
import hashlib
import json
import os
import random

import numpy as np

import zero_chain_amd as zk
from oracle import jubjub as jj
import helpers

S = jj.FS_MOD
SIGN = 1 << 255
OK, BAD_VK, BAD_R, BAD_S, BAD_EQUATION = 0, 1, 2, 3, 4
MESSAGE_LENGTHS = (0, 1, 32, 95, 96, 97, 223, 224, 225, 600)   # with the 32 bytes of Rbar in front: around BLAKE2b's 128-byte blocks
POOL_SIZE = 68


# ---------------------------------------------------------------------------------------------- the restatement
def generator():
    """FixedGenerators::Diversifier of the signing calls: in-tree index 1 (core/jubjub/src/curve/mod.rs:325-326)"""
    return jj.note_commitment_randomness_generator()


def h_star(a, b):
    """redjubjub.rs:24-26, util.rs:5-11: BLAKE2b-512 personalised, Fs::to_uniform"""
    return int.from_bytes(hashlib.blake2b(a + b, digest_size=64, person=b"Zcash_RedJubjubH").digest(), "little") % S


def sign(sk, t80, msg):
    """PrivateKey::sign (redjubjub.rs:73-103), the 80 random bytes given"""
    assert len(t80) == 80 and 0 <= sk < S
    r = h_star(t80, msg)
    rbar = jj.write_point(jj.mul(generator(), r))
    return rbar + ((r + h_star(rbar, msg) * sk) % S).to_bytes(32, "little")


def verify(vk, sig, msg):
    """PublicKey::read, then PublicKey::verify (redjubjub.rs:127-155): the reason code of the first test that fails"""
    key = jj.read_point(vk)
    if key is None:
        return BAD_VK
    c = h_star(sig[:32], msg)
    r = jj.read_point(sig[:32])
    if r is None:
        return BAD_R
    s = int.from_bytes(sig[32:], "little")
    if s >= S:
        return BAD_S
    g = generator()
    p = jj.add(jj.add(jj.mul(key, c), r), jj.mul((-g[0] % jj.R, g[1]), s))
    return OK if jj.double(jj.double(jj.double(p))) == jj.ZERO else BAD_EQUATION


# ---------------------------------------------------------------------------------------------- the pool
def enc_y(y, sign_bit=0):
    return (y | (SIGN if sign_bit else 0)).to_bytes(32, "little")


def scalar(v):
    return (v % S).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def order_eight_point():
    rng = random.Random(8)
    while True:
        p = jj.get_for_y(rng.randrange(jj.R), 0)
        if p is None:
            continue
        t = jj.mul(p, S)
        if jj.mul(t, 4) != jj.ZERO:
            assert jj.mul(t, 8) == jj.ZERO
            return t


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(helpers.GOLDEN, "redjubjub_keypair.json")) as f:
        v = json.load(f)
    return bytes.fromhex(v["rsk"]), bytes.fromhex(v["rvk"]), v["message"].encode()


@functools.lru_cache(maxsize=None)
def pool():
    """((vk, sig, msg, reason the restatement gives), ...): the refused cases at 0, 63, 64 and spread between the accepted ones"""
    rng = random.Random(1127)
    g = generator()
    rand_bytes = lambda n: bytes(rng.randrange(256) for _ in range(n))
    rand_fs = lambda: rng.randrange(1, S)
    good, bad = [], []

    def put(to, vk, sig, msg, stated):
        got = verify(vk, sig, msg)
        assert got == stated, "a constructed case gives reason %d, stated %d" % (got, stated)
        to.append((vk, sig, msg, got))

    def ordinary(length):
        sk, msg = rand_fs(), rand_bytes(length)
        return jj.write_point(jj.mul(g, sk)), sign(sk, rand_bytes(80), msg), msg

    # accepted, ordinary
    for length in MESSAGE_LENGTHS:
        put(good, *ordinary(length), OK)
    # accepted, the recoder's edges: S chosen, the key solved for
    for target in (0, 1, S - 1, (1 << 251) - 1):
        r, msg = rand_fs(), rand_bytes(40)
        rbar = jj.write_point(jj.mul(g, r))
        sk = (target - r) * pow(h_star(rbar, msg), -1, S) % S
        put(good, jj.write_point(jj.mul(g, sk)), rbar + scalar(target), msg, OK)
    # accepted by the cofactor
    t8 = order_eight_point()
    vk, sig, msg = ordinary(50)
    put(good, jj.write_point(jj.add(jj.read_point(vk), t8)), sig, msg, OK)
    sk, r, msg = rand_fs(), rand_fs(), rand_bytes(50)
    rbar = jj.write_point(jj.add(jj.mul(g, r), t8))
    put(good, jj.write_point(jj.mul(g, sk)), rbar + scalar(r + h_star(rbar, msg) * sk), msg, OK)
    for identity in (enc_y(1), enc_y(1, 1)):   # vk = O, S = r; the second with the sign bit set on x = 0
        r, msg = rand_fs(), rand_bytes(50)
        put(good, identity, jj.write_point(jj.mul(g, r)) + scalar(r), msg, OK)
    sk, msg = rand_fs(), rand_bytes(50)
    put(good, jj.write_point(jj.mul(g, sk)), enc_y(1) + scalar(h_star(enc_y(1), msg) * sk), msg, OK)   # Rbar = write(O), S = c sk
    # the reference's key pair
    rsk, rvk, msg = golden()
    assert jj.write_point(jj.mul(g, int.from_bytes(rsk, "little"))) == rvk
    put(good, rvk, sign(int.from_bytes(rsk, "little"), rand_bytes(80), msg), msg, OK)
    # refused
    flip = lambda b, i: bytes(b[:i]) + bytes([b[i] ^ 1]) + bytes(b[i + 1:])
    vk, sig, msg = ordinary(60)
    put(bad, vk, sig, flip(msg, 17), BAD_EQUATION)
    put(bad, vk, flip(sig, 32), msg, BAD_EQUATION)
    put(bad, vk, sig[:32] + (int.from_bytes(sig[32:], "little") + S).to_bytes(32, "little"), msg, BAD_S)
    put(bad, vk, sig[:32] + S.to_bytes(32, "little"), msg, BAD_S)
    assert jj.get_for_y(2, 0) is None
    not_in_field, no_x = enc_y(jj.R), enc_y(2)
    put(bad, vk, not_in_field + sig[32:], msg, BAD_R)
    put(bad, vk, no_x + sig[32:], msg, BAD_R)
    put(bad, not_in_field, sig, msg, BAD_VK)
    put(bad, no_x, sig, msg, BAD_VK)
    put(bad, no_x, not_in_field + sig[32:], msg, BAD_VK)   # both broken: the key is read first
    put(bad, ordinary(0)[0], sig, msg, BAD_EQUATION)       # another key
    while len(good) + len(bad) < POOL_SIZE:
        put(good, *ordinary(rng.randrange(0, 300)), OK)
    assert {c[3] for c in bad} == {BAD_VK, BAD_R, BAD_S, BAD_EQUATION}
    # refused at lanes 0, 63 and 64 (both sides of a block boundary), the others every fifth place
    at = [0, 63, 64] + [5 * k for k in range(1, len(bad) - 2)]
    assert len(set(at)) == len(bad) and max(at) < POOL_SIZE
    out, good_it, bad_it = [], iter(good), iter(bad)
    for i in range(POOL_SIZE):
        out.append(next(bad_it) if i in at else next(good_it))
    assert all(out[i][3] != OK for i in (0, 63, 64)) and len(out) <= 80
    return tuple(out)


# ---------------------------------------------------------------------------------------------- the entries
def raw_verify(lib, cases, device, with_reasons=True):
    """zk_redjubjub_verify_batch through the ctypes handle: (ok bytes, reason bytes), the outputs pre-filled with 0xAA"""
    n = len(cases)
    cat = lambda parts: np.frombuffer(b"".join(parts), dtype=np.uint8).copy() if parts and b"".join(parts) else np.zeros(1, dtype=np.uint8)
    vks, sigs, msgs = cat([c[0] for c in cases]), cat([c[1] for c in cases]), cat([c[2] for c in cases])
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c[2]) for c in cases])
    ok, why = np.full(max(n, 1), 0xAA, dtype=np.uint8), np.full(max(n, 1), 0xAA, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.check(lib.zk_redjubjub_verify_batch(n, ptr(vks), ptr(sigs), ptr(msgs), ptr(offs), -1 if device is None else device, ptr(ok),
                                            ptr(why) if with_reasons else None))
    return ok.tobytes()[:n], why.tobytes()[:n]


def verdicts_match(lib, cases, device):
    ok, why = raw_verify(lib, cases, device)
    for i, c in enumerate(cases):
        assert why[i] == c[3], "n = %d, signature %d: reason %d, expected %d" % (len(cases), i, why[i], c[3])
        assert ok[i] == (1 if c[3] == OK else 0)
    assert raw_verify(lib, cases, device, with_reasons=False)[0] == ok   # reason_out may be NULL
    # the host mirror
    got_ok, got_why = zk.redjubjub_verify([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], device=device, lib=lib)
    assert got_ok == [c[3] == OK for c in cases] and got_why == [c[3] for c in cases]
    return ok, why
