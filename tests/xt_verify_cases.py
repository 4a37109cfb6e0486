"""Transfer extrinsics judged from their bytes: IntoXY (zk_jubjub_into_xy) against oracle/jubjub.py, and the two transaction
entries (zk_confidential_verify_batch, zk_anonymous_verify_batch) against the oracle's inputs and verdicts.  Every function
takes `lib` (a ZkLib over one build of the C ABI), as tests/parity_cases.py does; `device` None = the host form."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import zero_chain_amd as zk
from zero_chain_amd import _lib as zl
from oracle import bls12_381 as bls
from oracle import jubjub as jj
import helpers

SIGN = 1 << 255
BATCH_SIZES = (1, 63, 64, 65, 715)   # 715 = 11 x 65: the points of 65 confidential transfers


def enc_y(y, sign=0):
    return (y | (SIGN if sign else 0)).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def expected(enc):
    """(status, 64 bytes) IntoXY must give for an encoding, from the oracle's curve."""
    v = int.from_bytes(enc, "little")
    if v & (SIGN - 1) >= jj.R:
        return 1, bytes(64)
    p = jj.read_point(enc)
    if p is None:
        return 2, bytes(64)
    if jj.mul(p, jj.FS_MOD) != jj.ZERO:
        return 3, bytes(64)
    return 0, p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def torsion_points():
    """Points of order 2, 4 and 8: multiples of [s]Q for a curve point Q with a full torsion component."""
    for y in (3, 5, 11, 13, 17, 19, 23):
        q = jj.get_for_y(y, 0)
        if q is None:
            continue
        t8 = jj.mul(q, jj.FS_MOD)
        if jj.mul(t8, 4) != jj.ZERO:
            t4, t2 = jj.double(t8), jj.mul(t8, 4)
            assert t2 == (0, jj.R - 1) and jj.double(t2) == jj.ZERO and jj.double(t4) == t2
            return t2, t4, t8
    raise AssertionError("no point of order 8 found")


@functools.lru_cache(maxsize=None)
def prime_order_points(n=40, seed=11):
    rng = random.Random(seed)
    gen = jj.note_commitment_randomness_generator()
    return tuple(jj.mul(gen, rng.randrange(1, jj.FS_MOD)) for _ in range(n))


@functools.lru_cache(maxsize=None)
def pool():
    """(accepted encodings, refused encodings): the issue's list, each with both values of the sign bit."""
    base = [jj.write_point(p) for p in prime_order_points()]
    base += [enc_y(1), enc_y(jj.R - 1), enc_y(jj.R), enc_y(SIGN - 1)]
    base += [enc_y(y) for y in (2, 4, 6)] + [enc_y(y) for y in (3, 5, 11)]
    p = prime_order_points()[0]
    for t in torsion_points():
        q = jj.add(p, t)
        base += [jj.write_point(q), jj.write_point(jj.mul(q, 8))]
    both = [bytes(e[:31] + bytes([e[31] ^ s])) for e in base for s in (0, 0x80)]
    good = [e for e in both if expected(e)[0] == 0]
    bad = [e for e in both if expected(e)[0] != 0]
    # what the issue states about these encodings, re-checked against the oracle
    assert all(expected(enc_y(y, s))[0] == 2 for y in (2, 4, 6) for s in (0, 1))
    assert all(expected(enc_y(y, s))[0] == 3 for y in (3, 5, 11) for s in (0, 1))
    assert expected(enc_y(jj.R))[0] == 1 and expected(enc_y(SIGN - 1))[0] == 1
    assert expected(enc_y(1, 1)) == (0, (0).to_bytes(32, "little") + (1).to_bytes(32, "little"))
    assert expected(enc_y(jj.R - 1))[0] == 3
    for t in torsion_points():
        assert expected(jj.write_point(jj.add(p, t)))[0] == 3 and expected(jj.write_point(jj.mul(jj.add(p, t), 8)))[0] == 0
    assert {expected(e)[0] for e in bad} == {1, 2, 3}
    return tuple(good), tuple(bad)


def batch(n, seed):
    """n encodings from the pool: refused ones at the first and last index and on both sides of a 64-lane boundary."""
    good, bad = pool()
    rng = random.Random(seed)
    out = [rng.choice(good + bad) if rng.random() < 0.3 else rng.choice(good) for _ in range(n)]
    for k, i in enumerate((0, n - 1, 63, 64)):
        if 0 <= i < n:
            out[i] = bad[(seed + 5 * k) % len(bad)]
    return out


def raw_into_xy(lib, encs, device):
    n = len(encs)
    pb = np.frombuffer(b"".join(encs), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
    xy, st = np.full(max(n, 1) * 64, 0xAA, dtype=np.uint8), np.full(max(n, 1), 0xAA, dtype=np.uint8)
    lib.check(lib.zk_jubjub_into_xy(pb.ctypes.data_as(C.c_void_p), n, -1 if device is None else device, xy.ctypes.data_as(C.c_void_p),
                                    st.ctypes.data_as(C.c_void_p)))
    return xy.tobytes()[:64 * n], [int(v) for v in st[:n]]


def into_xy_against_oracle(lib, device, sizes=BATCH_SIZES):
    """Every byte of xy_out and every status, at the batch sizes around a 64-lane block."""
    good, bad = pool()
    cases = [[good[0]], [good[1], good[2]]] + [batch(n, 100 + n) for n in sizes] + [list(good + bad)]
    for encs in cases:
        xy, st = raw_into_xy(lib, encs, device)
        want = [expected(e) for e in encs]
        for i, (e, (ws, wxy)) in enumerate(zip(encs, want)):
            assert st[i] == ws, "n = %d, point %d (%s): status %d, expected %d" % (len(encs), i, e.hex(), st[i], ws)
            assert xy[64 * i:64 * i + 64] == wxy, "n = %d, point %d (%s): coordinates differ" % (len(encs), i, e.hex())
    # nothing to do touches no buffer
    xy, st = raw_into_xy(lib, [], device)
    assert xy == b"" and st == []
    # the host mirror
    encs = [good[3], bad[0], good[4], bad[-1]]
    vals, st = zk.jubjub_into_xy(encs, device=device, lib=lib)
    assert st == [expected(e)[0] for e in encs]
    assert vals == [None if expected(e)[0] else jj.read_point(e) for e in encs]


# ----------------------------------------------------------------------------------------------
# verdicts on a small key: proofs from the trapdoor for chosen inputs
# ----------------------------------------------------------------------------------------------
CONF_FIELDS = zk.CONFIDENTIAL_XT_POINTS
PROOF_A, PROOF_B = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321


def vk_bytes_of(pk):
    """VerifyingKey::write bytes: the head of a Parameters file"""
    n_ic = int.from_bytes(pk[864:868], "big")
    return pk[:868 + 96 * n_ic]


@functools.lru_cache(maxsize=None)
def _proof_ab():
    return (bls.g1_compressed(bls.G1.to_affine(bls.G1.mul(bls.G1_GEN, PROOF_A))),
            bls.g2_compressed(bls.G2.to_affine(bls.G2.mul(bls.G2_GEN, PROOF_B))))


def trapdoor_proof(P, inputs):
    """A proof the key accepts for exactly these public inputs: c = (a b - alpha beta - gamma (ic[0] + sum x_i ic[i])) / delta"""
    sc, r = P.sc, bls.R_MOD
    assert len(inputs) + 1 == len(sc["ic"])
    acc = (sc["ic"][0] + sum(x * k for x, k in zip(inputs, sc["ic"][1:]))) % r
    c = (PROOF_A * PROOF_B - sc["alpha"] * sc["beta"] - sc["gamma"] * acc) * pow(sc["delta"], -1, r) % r
    a, b = _proof_ab()
    return a + b + bls.g1_compressed(bls.G1.to_affine(bls.G1.mul(bls.G1_GEN, c)))


def inputs_of(points):
    """the public inputs the reference's PublicInputBuilder forms, or None where IntoXY refuses one"""
    out = []
    for e in points:
        st, xy = expected(bytes(e))
        if st:
            return None
        out += [int.from_bytes(xy[:32], "little"), int.from_bytes(xy[32:], "little")]
    return out


def first_refusal(points, names):
    for name, e in zip(names, points):
        st = expected(bytes(e))[0]
        if st:
            return (name, zk.INTO_XY_REASONS[st])
    return None


def conf_xt(points, proof):
    """ConfidentialXt dict from the eleven encodings in push order (g_epoch, field 10, travels beside it)"""
    p = points
    return dict(proof=proof, enc_key_sender=p[0], enc_key_recipient=p[1], left_amount_sender=p[2], left_amount_recipient=p[3],
                right_randomness=p[4], left_fee=p[5], enc_balance=p[6] + p[7], rvk=p[8], nonce=p[10], rsk=bytes(32))


@functools.lru_cache(maxsize=None)
def small_conf_key():
    r1, asg, P, pk = helpers.small_case(31, 23, 6, 30)
    return P, vk_bytes_of(pk)


@functools.lru_cache(maxsize=None)
def good_conf(which=0):
    """(eleven encodings, proof): ten random prime-order points and one identity"""
    P, _ = small_conf_key()
    pts = [jj.write_point(p) for p in prime_order_points()[11 * which + 1:11 * which + 12]]
    pts[7] = enc_y(1)
    return tuple(pts), trapdoor_proof(P, inputs_of(pts))


def run_conf(lib, pvk, rows, shared_epoch=None, explicit_balances=False):
    """rows: (points, proof).  Returns (verdicts, refusals) of the entry and checks them against the oracle's inputs through
    verify_proofs of the same library."""
    xts = [conf_xt(list(pts), proof) for pts, proof in rows]
    if explicit_balances:   # the xt's own field must then be ignored
        bal = [(pts[6], pts[7]) for pts, _ in rows]
        for x in xts:
            x["enc_balance"] = enc_y(2) + enc_y(2)
    else:
        bal = None
    ge = shared_epoch if shared_epoch is not None else [pts[9] for pts, _ in rows]
    ok, ref = zk.verify_confidential_xts(pvk, xts, ge, enc_balances=bal)
    eff = [list(pts[:9]) + [shared_epoch if shared_epoch is not None else pts[9]] + [pts[10]] for pts, _ in rows]
    assert ref == [first_refusal(p, CONF_FIELDS) for p in eff]
    formed = [i for i, p in enumerate(eff) if inputs_of(p) is not None]
    want = [False] * len(rows)
    if formed:
        for i, v in zip(formed, zk.verify_proofs(pvk, [rows[i][1] for i in formed], [inputs_of(eff[i]) for i in formed])):
            want[i] = v
    assert ok == want
    return ok, ref


def confidential_verdicts(lib):
    P, vkb = small_conf_key()
    pvk = zk.prepare_verifying_key(vkb, lib=lib)
    try:
        assert pvk.n_inputs == 22
        pts, proof = good_conf(0)
        pts2, proof2 = good_conf(1)
        undecodable, other = enc_y(2), jj.write_point(prime_order_points()[30])
        torsion = jj.write_point(jj.add(prime_order_points()[0], torsion_points()[2]))
        assert expected(undecodable)[0] == 2 and expected(torsion)[0] == 3 and expected(other)[0] == 0

        def with_field(k, e):
            q = list(pts)
            q[k] = e
            return tuple(q)
        rows = [(pts, proof)]
        rows += [(with_field(k, undecodable), proof) for k in range(11)]
        rows += [(with_field(k, torsion), proof) for k in range(11)]
        two = list(pts)
        two[3], two[8] = torsion, undecodable
        rows.append((tuple(two), proof))
        rows.append((with_field(4, other), proof))
        flipped = bytearray(proof)
        flipped[150] ^= 1
        rows.append((pts, bytes(flipped)))
        rows.append((pts2, proof2))
        ok, ref = run_conf(lib, pvk, rows)
        assert ok[0] and ok[-1] and not any(ok[1:-1])
        for k in range(11):
            assert ref[1 + k] == (CONF_FIELDS[k], "not on the curve") and ref[12 + k] == (CONF_FIELDS[k], "not in the prime-order subgroup")
        assert ref[23] == (CONF_FIELDS[3], "not in the prime-order subgroup")
        assert ref[24] is None and ref[25] is None and ref[0] is None and ref[26] is None

        # sizes, good and bad transactions at known indices
        bad_row = (with_field(10, undecodable), proof)
        wrong_row = (pts, proof2)
        for n in (1, 3, 65):
            batch_rows = [(pts, proof) if i % 2 == 0 else (pts2, proof2) for i in range(n)]
            marks = {}
            if n > 1:
                marks = {1: bad_row, n - 1: wrong_row}
                if n > 64:
                    marks.update({63: wrong_row, 64: bad_row})
            for i, r in marks.items():
                batch_rows[i] = r
            ok, ref = run_conf(lib, pvk, batch_rows)
            assert ok == [i not in marks for i in range(n)]
            assert [i for i in range(n) if ref[i]] == sorted(i for i, r in marks.items() if r is bad_row)

        # one shared g_epoch (decoded once) against one per xt: two different epochs
        same_epoch = [(pts, proof), (pts, proof), (pts, proof)]
        ok0, _ = run_conf(lib, pvk, same_epoch, shared_epoch=pts[9])
        ok1, _ = run_conf(lib, pvk, same_epoch)
        assert ok0 == ok1 == [True] * 3
        ok0, _ = run_conf(lib, pvk, [(pts, proof), (pts2, proof2)], shared_epoch=pts[9])   # the second was made for another epoch
        assert ok0 == [True, False]
        ok1, _ = run_conf(lib, pvk, [(pts, proof), (pts2, proof2)])
        assert ok1 == [True, True]
        # a refused shared g_epoch refuses every xt with field 10
        for e, reason in ((undecodable, "not on the curve"), (torsion, "not in the prime-order subgroup")):
            ok, ref = run_conf(lib, pvk, [(pts, proof), (pts2, proof2)], shared_epoch=e)
            assert ok == [False, False] and ref == [("g_epoch", reason)] * 2
        # the chain's stored balances beside the xts against each xt's own field
        mixed = [(pts, proof), bad_row, (pts2, proof2), (with_field(6, torsion), proof)]
        assert run_conf(lib, pvk, mixed, explicit_balances=True) == run_conf(lib, pvk, mixed)
        # the array of structures gen_proofs(raw=True) returns is taken as it is
        arr = (zl.ConfidentialXt * 2)()
        for dst, (p, pf) in zip(arr, [(pts, proof), (pts2, proof2)]):
            for f, v in conf_xt(list(p), pf).items():
                getattr(dst, f)[:] = v
        assert zk.verify_confidential_xts(pvk, arr, [pts[9], pts2[9]]) == ([True, True], [None, None])
        # n = 0
        assert zk.verify_confidential_xts(pvk, [], pts[9]) == ([], [])
        st = lib.zk_confidential_verify_batch(pvk._h, 0, None, None, None, 0, None, None)
        assert st == 0
    finally:
        pvk.close()
    # a key with 3 inputs
    r1, asg, P3, pk3 = helpers.small_case(1, 4, 6, 9)
    pvk3 = zk.prepare_verifying_key(vk_bytes_of(pk3), lib=lib)
    try:
        assert pvk3.n_inputs == 3
        for fn, args in ((zk.verify_confidential_xts, ([conf_xt(list(pts), proof)], pts[9])),
                         (zk.verify_anonymous_xts, ([anon_xt(list(anon_points()), proof)], pts[9], [anon_balances(anon_points())]))):
            with pytest.raises(zk.ZkError) as e:
                fn(pvk3, *args)
            assert e.value.variant == "MalformedVerifyingKey"
    finally:
        pvk3.close()


# ---- the anonymous entry: 52 points, 104 inputs
ANON_FIELDS = zk.ANONYMOUS_XT_POINTS


def anon_points():
    """52 encodings in push order from a handful of prime-order points"""
    good = [jj.write_point(p) for p in prime_order_points()]
    return tuple(good[(3 * i + 1) % len(good)] for i in range(52))


def anon_xt(p, proof):
    return dict(proof=proof, enc_keys=list(p[0:12]), left_ciphertexts=list(p[12:24]), right_ciphertext=p[48], rvk=p[49], nonce=p[51],
                rsk=bytes(32))


def anon_balances(p):
    return [(p[24 + m], p[36 + m]) for m in range(12)]


def anonymous_verdicts(lib):
    r1, asg, P, pk = helpers.small_case(32, 105, 6, 30)
    pvk = zk.prepare_verifying_key(vk_bytes_of(pk), lib=lib)
    try:
        assert pvk.n_inputs == 104
        p = anon_points()
        proof = trapdoor_proof(P, inputs_of(p))
        bad = list(p)
        bad[36] = enc_y(4)   # field 37: the first balance right
        xts = [anon_xt(list(p), proof), anon_xt(bad, proof)]
        ok, ref = zk.verify_anonymous_xts(pvk, xts, p[50], [anon_balances(p), anon_balances(bad)])
        assert ANON_FIELDS[36] == "enc_balances_right[0]" and len(ANON_FIELDS) == 52
        assert ok == [True, False] and ref == [None, (ANON_FIELDS[36], "not on the curve")]
        assert zk.verify_proofs(pvk, [proof], [inputs_of(p)]) == [True]
        # one epoch per xt, the second a different valid point: formed, not accepted
        ok, ref = zk.verify_anonymous_xts(pvk, [xts[0], xts[0]], [p[50], p[0]], [anon_balances(p)] * 2)
        assert ok == [True, False] and ref == [None, None]
        assert zk.verify_anonymous_xts(pvk, [], p[50], []) == ([], [])
    finally:
        pvk.close()


# ----------------------------------------------------------------------------------------------
# the reference's own vector (modules/encrypted-balances/src/lib.rs:438-464: must not verify)
# ----------------------------------------------------------------------------------------------
def reference_vector(lib):
    with open(os.path.join(helpers.GOLDEN, "zk_system_vectors.json")) as f:
        v = json.load(f)["test_call_with_wrong_proof"]
    h = lambda name: bytes.fromhex(v[name])
    data = open(os.path.join(helpers.GOLDEN, "conf_vk.dat"), "rb").read()
    pvk = zk.PreparedVerifyingKey.read(data, lib=lib)
    try:
        assert pvk.n_inputs == 22
        nine = [h(n) for n in ("pkd_addr_alice", "pkd_addr_bob", "enc10_by_alice", "enc10_by_bob", "enc1_by_alice", "randomness", "rvk",
                               "nonce", "g_epoch")]
        assert [expected(e)[0] for e in nine] == [0] * 9   # all nine decode and lie in the subgroup
        xt = dict(proof=h("proof"), enc_key_sender=h("pkd_addr_alice"), enc_key_recipient=h("pkd_addr_bob"), left_amount_sender=h("enc10_by_alice"),
                  left_amount_recipient=h("enc10_by_bob"), left_fee=h("enc1_by_alice"), right_randomness=h("randomness"), rvk=h("rvk"),
                  nonce=h("nonce"), rsk=bytes(32), enc_balance=bytes(64))
        ok, ref = zk.verify_confidential_xts(pvk, [xt], h("g_epoch"), enc_balances=[zk.ZERO_CIPHERTEXT])
        assert ref == [None] and ok == [False]
    finally:
        pvk.close()
