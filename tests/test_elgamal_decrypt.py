"""ElGamal balance decryption (zk_elgamal_table_create / zk_elgamal_decrypt / zk_elgamal_table_free, csrc/elgamal_dlog.h):
the reference's Ciphertext::decrypt (core/proofs/src/no_std_aliases/elgamal.rs:85-108) as a baby-step giant-step search on
the device; Ciphertext::add / sub (:139-158, zk_elgamal_add); the balance query of zface (zface/src/utils/getter.rs:135-174).
CPU: the x86 emulation build of the kernel sources with 8 baby-step bits.  GPU: the product library with the default 20."""
import ctypes as C
import random

import pytest

from oracle import jubjub as jj
from oracle import synth

G = jj.note_commitment_randomness_generator()
IDENTITY = jj.write_point(jj.ZERO)
LIMIT = 1000000


def reference_decrypt(left, right, dec_key, limit):
    """elgamal.rs:92-107 restated: v = left - dk right; acc = O, O + G, ... compared with v, `limit` times."""
    sr = jj.mul(right, dec_key)
    v = jj.add(left, ((-sr[0]) % jj.R, sr[1]))
    acc = jj.ZERO
    for i in range(limit):
        if acc == v:
            return i
        acc = jj.add(acc, G)
    return None


def fs(seed, n):
    rng = synth.SplitMix64(seed)
    return [rng.field(jj.FS_MOD) for _ in range(n)]


def encrypt(lib, values, dec_keys, seed=5):
    """ciphertexts of `values` under the encryption keys of `dec_keys` (zk_jubjub_base_mul and zk_elgamal_encrypt, which
    tests/test_gen_proof.py holds to the oracle)"""
    import zero_chain_amd as zk
    return zk.elgamal_encrypt(values, fs(seed, len(values)), zk.jubjub_base_mul(dec_keys, lib=lib), lib=lib)


def neg(p):
    return ((-p[0]) % jj.R, p[1])


# ---------------------------------------------------------------------------------------------- CPU (emulation build)
def test_small_table_finds_exactly_the_values_below_the_limit(emu_lib):
    import zero_chain_amd as zk
    dk = fs(1, 1)[0]
    found, missing = [0, 1, 255, 256, 257, 511, 512, 4999], [5000, 5001, 70000]
    vals = found + missing
    left, right = encrypt(emu_lib, vals, [dk] * len(vals))
    want = found + [None] * len(missing)
    with zk.ElGamalTable(8, lib=emu_lib) as t:
        assert t.decrypt(left, right, dk, limit=5000) == want                       # one key for all
        assert t.decrypt(left, right, [dk] * len(vals), limit=5000) == want         # one key each
        assert t.decrypt(left, right, dk, limit=256) == [0, 1, 255] + [None] * 8    # limit <= 2^8: one probe each
        assert t.decrypt(left, right, dk, limit=1) == [0] + [None] * 10
        assert t.decrypt([], [], dk) == []
    for k in (vals.index(257), vals.index(5001)):   # the reference's own loop agrees
        assert reference_decrypt(jj.read_point(left[k]), jj.read_point(right[k]), dk, 5000) == want[k]


def test_keys_zero_ciphertext_and_wrong_key(emu_lib):
    import zero_chain_amd as zk
    dks = fs(2, 4)
    vals = [7, 300, 4321, 12]
    left, right = encrypt(emu_lib, vals, dks)
    with zk.ElGamalTable(8, lib=emu_lib) as t:
        assert t.decrypt(left, right, dks, limit=5000) == vals
        wrong = [dks[0], dks[2], dks[2], dks[3]]
        assert t.decrypt(left, right, wrong, limit=5000) == [7, None, 4321, 12]
        assert t.decrypt(left, right, dks[0], limit=5000) == [7, None, None, None]
        # Ciphertext::zero() decrypts to 0 under any key
        assert t.decrypt([IDENTITY, IDENTITY], [IDENTITY, IDENTITY], dks[:2], limit=5000) == [0, 0]


def test_wallet_chain_decrypts_its_own_balance(emu_lib):
    """spending key -> dec_key_sender (zk_transfer_derive) -> a ciphertext under enc_key_sender -> its amount"""
    import zero_chain_amd as zk
    import test_gen_proof as tg
    rq, _ = tg.reference_request(1)   # Alice's balance of the reference's test: 100, randomness one (lib.rs:372-420)
    st, _ = zk.transfer_derive(zk.transfer_requests([rq]), lib=emu_lib)
    dk = int.from_bytes(bytes(st[0].dec_key_sender), "little")
    (enc_key,) = zk.jubjub_base_mul([dk], lib=emu_lib)
    left, right = zk.elgamal_encrypt([91], [123456789], [enc_key], lib=emu_lib)
    with zk.ElGamalTable(8, lib=emu_lib) as t:
        assert t.decrypt([rq["enc_balance_left"], left[0]], [rq["enc_balance_right"], right[0]], dk, limit=5000) == [100, 91]


def test_add_subtract_and_balance_query(emu_lib):
    import zero_chain_amd as zk
    dk = fs(3, 1)[0]
    a, b = [40, 7, 1000, 3], [2, 7, 999, 4]
    la, ra = encrypt(emu_lib, a, [dk] * 4, seed=6)
    lb, rb = encrypt(emu_lib, b, [dk] * 4, seed=7)
    ls, rs = zk.elgamal_add(la, ra, lb, rb, lib=emu_lib)
    ld, rd = zk.elgamal_add(la, ra, lb, rb, subtract=True, lib=emu_lib)
    for k in range(4):
        pa, qa, pb, qb = (jj.read_point(x[k]) for x in (la, ra, lb, rb))
        assert (ls[k], rs[k]) == (jj.write_point(jj.add(pa, pb)), jj.write_point(jj.add(qa, qb)))
        assert (ld[k], rd[k]) == (jj.write_point(jj.add(pa, neg(pb))), jj.write_point(jj.add(qa, neg(qb))))
    with zk.ElGamalTable(8, lib=emu_lib) as t:
        assert t.decrypt(ls, rs, dk, limit=5000) == [42, 14, 1999, 7]
        assert t.decrypt(ld, rd, dk, limit=5000) == [38, 0, 1, None]   # a < b: no amount below the limit
        # getter.rs:163-167: balance + pending transfer, an absent part counting as Ciphertext::zero()
        assert zk.balance_query(dk, la[0] + ra[0], (lb[0], rb[0]), table=t, limit=5000) == (42, ls[0] + rs[0])
        assert zk.balance_query(dk, la[2] + ra[2], table=t, limit=5000) == (1000, la[2] + ra[2])
        assert zk.balance_query(dk, None, lb[3] + rb[3], table=t, limit=5000) == (4, lb[3] + rb[3])
        assert zk.balance_query(dk, table=t, limit=5000) == (0, IDENTITY * 2)


def test_refusals(emu_lib):
    import zero_chain_amd as zk
    x, y = jj.mul(G, 0x1234567)
    torsion = jj.write_point(((-x) % jj.R, (-y) % jj.R))   # (-x, -y) = P + (0, -1): on the curve, order 2 s
    not_a_point = bytes([0xff] * 32)
    dk = fs(4, 1)[0]
    left, right = encrypt(emu_lib, [1, 2], [dk, dk])
    for bits in (7, 25, 1000):
        with pytest.raises(zk.ZkError) as e:
            zk.ElGamalTable(bits, lib=emu_lib)
        assert e.value.variant == "InvalidArgument" and "baby_bits" in str(e.value)
    with zk.ElGamalTable(8, lib=emu_lib) as t:
        for limit in (0, (1 << 32) + 1, 1 << 40):
            with pytest.raises(zk.ZkError) as e:
                t.decrypt(left, right, dk, limit=limit)
            assert e.value.variant == "InvalidArgument" and "limit" in str(e.value)
        cases = [
            ([left[0], not_a_point], right, dk, "ciphertext 1: left is not a Jubjub point"),
            (left, [right[0], torsion], dk, "ciphertext 1: right is not in the prime-order subgroup"),
            ([torsion, left[1]], right, dk, "ciphertext 0: left is not in the prime-order subgroup"),
            (left, right, jj.FS_MOD, "dec_key is not a canonical Fs scalar"),
            (left, right, [dk, jj.FS_MOD], "dec_key 1 is not a canonical Fs scalar"),
        ]
        for l, r, k, what in cases:
            with pytest.raises(zk.ZkError) as e:
                t.decrypt(l, r, k, limit=5000)
            assert e.value.variant == "InvalidArgument" and what in str(e.value)
        # the raw entry: NULL pointers with n > 0, a stride other than 0 / 32; n = 0 is fine with NULLs
        buf = lambda b: C.create_string_buffer(bytes(b), len(b))
        L, R, K = buf(b"".join(left)), buf(b"".join(right)), buf(zk.scalars_to_bytes([dk, dk]).tobytes())
        vals, found = (C.c_uint32 * 2)(), (C.c_uint8 * 2)()
        dec = emu_lib.zk_elgamal_decrypt
        assert dec(t._h, 2, L, R, K, 32, 5000, vals, found) == 0 and list(vals) == [1, 2] and list(found) == [1, 1]
        for args, what in (((None, 2, L, R, K, 32), "null"), ((t._h, 2, None, R, K, 32), "null"), ((t._h, 2, L, None, K, 32), "null"),
                           ((t._h, 2, L, R, None, 32), "null"), ((t._h, 2, L, R, K, 16), "dec_key_stride"),
                           ((t._h, 2, L, R, K, 64), "dec_key_stride")):
            with pytest.raises(zk.ZkError) as e:
                emu_lib.check(dec(*args, 5000, vals, found))
            assert e.value.variant == "InvalidArgument" and what in str(e.value)
        for out in ((None, found), (vals, None)):
            with pytest.raises(zk.ZkError):
                emu_lib.check(dec(t._h, 2, L, R, K, 32, 5000, *out))
        assert dec(t._h, 0, None, None, None, 0, 5000, None, None) == 0
    # zk_elgamal_add reads both ciphertexts as Ciphertext::read does
    with pytest.raises(zk.ZkError) as e:
        zk.elgamal_add(left, right, [left[0], torsion], right, lib=emu_lib)
    assert e.value.variant == "InvalidArgument" and "ciphertext 1: left_b is not in the prime-order subgroup" in str(e.value)
    with pytest.raises(zk.ZkError) as e:
        zk.elgamal_add(left, [not_a_point, right[1]], left, right, subtract=True, lib=emu_lib)
    assert "ciphertext 0: right_a is not a Jubjub point" in str(e.value)
    with pytest.raises(zk.ZkError):
        emu_lib.check(emu_lib.zk_elgamal_add(None, None, None, None, 1, 0, None, None))
    assert zk.elgamal_add([], [], [], [], lib=emu_lib) == ([], [])


def test_the_lowest_failing_index_is_reported_whatever_the_thread_count(emu_lib):
    """The host entries fan out over contiguous ranges (host_common.h for_each_status): with one thread and with eight - the two
    bad items then lie in different ranges, the higher one in an earlier position of its range - the caller hears of the lower."""
    import zero_chain_amd as zk
    scalars = list(range(1, 201))
    scalars[150] = scalars[30] = jj.FS_MOD
    left, right = encrypt(emu_lib, [1], fs(6, 1))
    lefts = [left[0]] * 100
    lefts[90] = lefts[12] = bytes([0xff] * 32)
    try:
        for threads in (1, 8):
            zk.set_host_threads(threads, lib=emu_lib)
            with pytest.raises(zk.ZkError) as e:
                zk.jubjub_base_mul(scalars, lib=emu_lib)
            assert e.value.variant == "InvalidArgument" and "scalar 30 is not a canonical Fs scalar" in str(e.value), threads
            with pytest.raises(zk.ZkError) as e:
                zk.elgamal_add(lefts, right * 100, [left[0]] * 100, right * 100, lib=emu_lib)
            assert e.value.variant == "InvalidArgument" and "ciphertext 12: left_a is not a Jubjub point" in str(e.value), threads
    finally:
        zk.set_host_threads(0, lib=emu_lib)


def test_fingerprint_collisions_change_no_result(emu_lib, monkeypatch):
    """ZKAMD_DEBUG_DLOG_FP_BITS (test hooks only) narrows the fingerprint of a hash slot: with 0 bits every occupied slot
    a probe passes is a fingerprint hit that only the full coordinates can tell apart."""
    import zero_chain_amd as zk
    dk = fs(5, 1)[0]
    vals = [0, 1, 200, 255, 256, 3000, 4999, 5000, 9000]
    left, right = encrypt(emu_lib, vals, [dk] * len(vals))
    want = {lim: [v if v < lim else None for v in vals] for lim in (256, 5000)}
    for bits in ("0", "2"):
        monkeypatch.setenv("ZKAMD_DEBUG_DLOG_FP_BITS", bits)
        with zk.ElGamalTable(8, lib=emu_lib) as t:   # (read when the table is built)
            for lim in (256, 5000):
                assert t.decrypt(left, right, dk, limit=lim) == want[lim], (bits, lim)


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def table(gpu_lib):
    import zero_chain_amd as zk
    t = zk.ElGamalTable(lib=gpu_lib)
    yield t
    t.close()


@pytest.mark.gpu
def test_gpu_reference_limit(gpu_lib, table):
    dk = fs(10, 1)[0]
    vals = [0, 1, 999999, 1000000, (1 << 20) - 1, 1 << 20, (1 << 32) - 1]
    left, right = encrypt(gpu_lib, vals, [dk] * len(vals))
    assert table.decrypt(left, right, dk) == [0, 1, 999999, None, None, None, None]
    assert table.decrypt(left[:2], right[:2], dk, limit=1) == [0, None]


@pytest.mark.gpu
def test_gpu_every_u32(gpu_lib, table):
    rng = random.Random(11)
    dk = fs(11, 1)[0]
    vals = [1000000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 31, (1 << 32) - 1] + [rng.getrandbits(32) for _ in range(1024)]
    left, right = encrypt(gpu_lib, vals, [dk] * len(vals))
    assert table.decrypt(left[:1], right[:1], dk, limit=1 << 32) == vals[:1]
    assert table.decrypt(left, right, dk, limit=1 << 32) == vals
    # a limit between: every value below it, nothing above
    assert table.decrypt(left[:6], right[:6], dk, limit=(1 << 31) + 1) == vals[:5] + [None]


@pytest.mark.gpu
def test_gpu_batch_with_a_key_each(gpu_lib, table):
    rng = random.Random(12)
    dks = fs(12, 4096)
    vals = [rng.randrange(LIMIT) if i % 3 else rng.randrange(LIMIT, 1 << 32) for i in range(4096)]
    left, right = encrypt(gpu_lib, vals, dks)
    assert table.decrypt(left, right, dks) == [v if v < LIMIT else None for v in vals]
    assert table.decrypt(left[:256], right[:256], dks[:256], limit=1 << 32) == vals[:256]


@pytest.mark.gpu
def test_gpu_balance_query_feeds_a_transfer_that_verifies(gpu_lib, table):
    """getter.rs:135-174 then commands.rs:85-113: the decrypted sum is the request's balance, the summed ciphertext its
    enc_balance; gen_proof's own check_proof accepts the proof (a wrong balance would fail it with Unsatisfiable)."""
    import zero_chain_amd as zk
    import helpers
    import test_gen_proof as tg
    rq, _ = tg.reference_request(2)
    st, _ = zk.transfer_derive(zk.transfer_requests([rq]), lib=gpu_lib)
    dk = int.from_bytes(bytes(st[0].dec_key_sender), "little")
    (enc_key,) = zk.jubjub_base_mul([dk], lib=gpu_lib)
    (pl,), (pr,) = zk.elgamal_encrypt([5], [987654321], [enc_key], lib=gpu_lib)
    value, enc_total = zk.balance_query(dk, rq["enc_balance_left"] + rq["enc_balance_right"], pl + pr, table=table)
    assert value == 105
    mats = zk.ConstraintMatrices.transfer_circuit(lib=gpu_lib)
    params = pvk = None
    try:
        params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=gpu_lib)
        pvk = zk.prepare_verifying_key(params)
        good = dict(rq, amount=8, fee=1, remaining_balance=value - 9, enc_balance_left=enc_total[:32], enc_balance_right=enc_total[32:])
        (xt,) = zk.gen_proofs(params, mats, pvk, zk.transfer_requests([good]), [(3, 4)])
        assert len(xt["proof"]) == 192
        with pytest.raises(zk.ZkError) as e:   # the balance before the pending transfer does not add up
            zk.gen_proofs(params, mats, pvk, zk.transfer_requests([dict(good, remaining_balance=100 - 9)]), [(3, 4)])
        assert e.value.variant == "Unsatisfiable"
    finally:
        for h in (pvk, params, mats):
            if h is not None:
                h.close()


@pytest.mark.gpu
def test_gpu_memory_is_returned_and_wiped(gpu_lib):
    import zero_chain_amd as zk
    dk = fs(13, 1)[0]
    left, right = encrypt(gpu_lib, [5, 123456789], [dk, dk])
    before = zk.memory_stats(lib=gpu_lib)
    with zk.ElGamalTable(lib=gpu_lib) as t:
        held = zk.memory_stats(lib=gpu_lib)["device_held"] - before["device_held"]
        assert held >= (64 + 16) << 20, held
        assert t.decrypt(left, right, dk) == [5, None]
        assert t.decrypt(left, right, dk, limit=1 << 32) == [5, 123456789]
    after = zk.memory_stats(lib=gpu_lib)
    assert after["device_held"] == before["device_held"]
    assert after["device_released"] == after["device_wiped"] > before["device_released"]


@pytest.mark.gpu
def test_gpu_fingerprint_collisions_change_no_result(gpu_hooks_lib, monkeypatch):
    import zero_chain_amd as zk
    rng = random.Random(14)
    dk = fs(14, 1)[0]
    vals = [0, 999999, 1000000, 1 << 20, (1 << 32) - 1] + [rng.getrandbits(32) for _ in range(64)]
    left, right = encrypt(gpu_hooks_lib, vals, [dk] * len(vals))
    monkeypatch.setenv("ZKAMD_DEBUG_DLOG_FP_BITS", "0")
    with zk.ElGamalTable(lib=gpu_hooks_lib) as t:
        assert t.decrypt(left, right, dk) == [v if v < LIMIT else None for v in vals]
        assert t.decrypt(left, right, dk, limit=1 << 32) == vals
