"""ElGamal encryption of groups of keys as a stage with a device form (zk_elgamal_encrypt_dev; csrc/elgamal_encrypt.h) against the
Python model of tests/encrypt_cases.py: left = v G + r pk, right = r G on oracle.jubjub integers.

Every case runs on the x86 emulation build and, marked gpu, on the product library, each time with the host form forced
(ZKAMD_ENCRYPT_HOST_MAX large) and with the kernels forced (0): the two forms must write the same bytes and the same statuses, and
refuse the same arguments with the same message.  The model checks at most about 40 points per test (a multiplication in Python
each, computed once per distinct point); larger calls compare the two forms and hold the model to their first and last group.
No test runs more than about 520 lanes of a kernel: the largest is 40 groups of 12 keys - 480 variable-base, 12 decode, 40 + 80
fixed-base and 520 combine lanes."""
import ctypes as C

import numpy as np
import pytest

import anon_derive_cases as ad
import encrypt_cases as ec
import scan_cases as sc
from oracle import jubjub as jj

HOST, DEVICE = str(1 << 40), "0"
VAR = "ZKAMD_ENCRYPT_HOST_MAX"
STAGES = ("encrypt_points", "encrypt_combine")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "gpu_lib")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks_lib(request):
    """a build that reads the test hooks: the emulation build, or the product sources with -DZK_TEST_HOOKS"""
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "gpu_hooks_lib")


def both_forms(monkeypatch, lib, call):
    """(lefts, rights, statuses) of the call, the same from both forms"""
    import zero_chain_amd as zk
    values, rnd, enc, k = call
    monkeypatch.setenv(VAR, HOST)
    host = zk.elgamal_encrypt_dev(values, rnd, enc, k=k, lib=lib)
    monkeypatch.setenv(VAR, DEVICE)
    device = zk.elgamal_encrypt_dev(values, rnd, enc, k=k, lib=lib)
    assert host == device
    # device < 0 is the host form whatever the variable says
    assert zk.elgamal_encrypt_dev(values, rnd, enc, k=k, device=-1, lib=lib) == device
    return device


def check(monkeypatch, lib, call, groups=None):
    """both forms, and the model for `groups` (default: all)"""
    values, rnd, enc, k = call
    lefts, rights, statuses = both_forms(monkeypatch, lib, call)
    assert (len(lefts), len(rights), len(statuses)) == (len(rnd) * k, len(rnd), len(rnd) * k)
    for i in range(len(rnd)) if groups is None else groups:
        want = ec.expected_group(values, rnd, enc, k, i)
        assert (lefts[i * k:(i + 1) * k], rights[i], statuses[i * k:(i + 1) * k]) == want, i
    return lefts, rights, statuses


# ---------------------------------------------------------------------------------------------- shapes
def test_one_ciphertext(lib, monkeypatch):
    check(monkeypatch, lib, ([1234567], ec.randomness(1, 1), ec.keys(0, 1), 1))


def test_confidential_groups(lib, monkeypatch):
    """k = 3 as (amount, amount, fee) under (sender, recipient, sender): a repeated key inside a group"""
    call = ec.confidential(2, 2)
    assert call[2][0] == call[2][2] != call[2][1]
    check(monkeypatch, lib, call)


def test_anonymous_group(lib, monkeypatch):
    """k = 12 with -a, +a and ten zeros"""
    call = ec.anonymous(3, 1)
    assert sorted(v != 0 for v in call[0]) == [False] * 10 + [True] * 2 and sum(call[0]) == 0
    check(monkeypatch, lib, call)


def test_sixteen_keys(lib, monkeypatch):
    check(monkeypatch, lib, ([(-1) ** j * (j + 1) * 1000 for j in range(16)], ec.randomness(4, 1), ec.keys(5, 16), 16))


def test_the_old_entry_writes_the_same_bytes(lib, monkeypatch):
    """k = 1, v >= 0: zk_elgamal_encrypt on the same items"""
    import zero_chain_amd as zk
    values, rnd, enc = [0, 1, 77, ec.TOP, 1 << 30], ec.randomness(5, 5), ec.keys(9, 5)
    lefts, rights, statuses = both_forms(monkeypatch, lib, (values, rnd, enc, 1))
    assert statuses == [0] * 5
    assert (lefts, rights) == zk.elgamal_encrypt(values, rnd, enc, lib=lib)


# ---------------------------------------------------------------------------------------------- edges
def test_value_edges(lib, monkeypatch):
    """0 (no fixed-base value lane: left = [r]pk), +-1, +-(2^32 - 1), +-2^30 (only the sixth window is not zero); one group per
    value, all under one key and one randomness, so that lefts differ by the value alone; and a call whose values are all zero (k = 2,
    one group): left_j = [r]pk_j"""
    values = [0, 1, -1, ec.TOP, -ec.TOP, 1 << 30, -(1 << 30)]
    r, key = ec.randomness(6, 1)[0], ec.keys(20, 1)[0]
    lefts, rights, _ = check(monkeypatch, lib, (values, [r] * 7, [key] * 7, 1))
    assert len(set(lefts)) == 7 and len(set(rights)) == 1
    assert lefts[0] == jj.write_point(jj.mul(jj.read_point(key), r))
    # the same as ONE group of seven keys
    lefts7, rights7, _ = check(monkeypatch, lib, (values, [r], [key] * 7, 7))
    assert lefts7 == lefts and rights7 == rights[:1]
    # every value zero: the descriptors end in the group's padding, with no value lane behind it
    keys2 = ec.keys(21, 2)
    lefts0, _, _ = check(monkeypatch, lib, ([0, 0], [r], keys2, 2))
    assert lefts0 == [jj.write_point(jj.mul(jj.read_point(key_j), r)) for key_j in keys2]


def test_scalar_edges(lib, monkeypatch):
    """r = 0: right is the identity and left = [v]G; r = 1: left = [v]G + pk; r = s - 1; the identity as a key: accepted, left = [v]G"""
    key = ec.keys(30, 1)[0]
    values = [5, -5, 0, 9, 9, 7, -7]
    rnd = [0, 0, 0, 1, ec.S - 1, ec.randomness(7, 1)[0], ec.S - 1]
    enc = [key, key, key, key, key, ec.IDENTITY, ec.IDENTITY]
    lefts, rights, statuses = check(monkeypatch, lib, (values, rnd, enc, 1))
    assert statuses == [0] * 7
    assert rights[:3] == [ec.IDENTITY] * 3
    assert lefts[:3] == [jj.write_point(ec.base_mul(5)), jj.write_point(ec.base_mul(-5)), ec.IDENTITY]
    assert lefts[3] == jj.write_point(jj.add(ec.base_mul(9), jj.read_point(key))) and rights[3] == jj.write_point(ec.G)
    assert rights[4] == jj.write_point(sc.neg(ec.G))
    assert lefts[5:] == [jj.write_point(ec.base_mul(7)), jj.write_point(ec.base_mul(-7))]


def test_refusals_are_statuses(lib, monkeypatch):
    """y not in the field, y with no x, a torsion component, a good key: 1, 2, 3, 0 - the refused lefts zero, the good left and
    the right the model's; a second, clean group is unaffected, and so is a group whose refused key is repeated"""
    good = ec.keys(40, 5)
    bad = [sc.NOT_A_POINT, sc.off_curve(), sc.torsion()]
    enc = bad + good[:1] + good[1:5] + [bad[2], good[0], bad[2], ad.SMALL_ORDER]
    values = [3, -4, 5, 6, 10, 0, -12, 13, 1, 2, 0, 4]
    call = (values, ec.randomness(8, 3), enc, 4)
    lefts, rights, statuses = check(monkeypatch, lib, call)
    assert statuses == [1, 2, 3, 0] + [0] * 4 + [3, 0, 3, 3]
    assert lefts[:3] == [ec.ZERO_BYTES] * 3 and ec.ZERO_BYTES not in lefts[3:8]
    assert [lefts[i] == ec.ZERO_BYTES for i in range(8, 12)] == [True, False, True, True]
    assert all(r != ec.ZERO_BYTES for r in rights)


# ---------------------------------------------------------------------------------------------- arguments
PATTERN = 0xa5


def _raw_call(lib, n, k, values, rnd, enc, device=0, null=()):
    """the entry on buffers filled with PATTERN: (status, left, right, statuses)"""
    import zero_chain_amd as zk
    vb = np.asarray([int(v) for v in values], dtype=np.int64)
    rb = zk.scalars_to_bytes(rnd)
    kb = np.frombuffer(b"".join(enc), dtype=np.uint8).copy()
    nk = max(n * k, 1)
    left, right, st = (np.full(m, PATTERN, dtype=np.uint8) for m in (32 * nk, 32 * max(n, 1), nk))
    ptr = lambda name, a: None if name in null else a.ctypes.data_as(C.c_void_p)
    rc = lib.zk_elgamal_encrypt_dev(n, k, ptr("values", vb), ptr("randomness", rb), ptr("enc_keys", kb), device, ptr("left", left), ptr("right", right),
                                    ptr("status", st))
    return rc, left, right, st


def _refused(monkeypatch, lib, text, n, k, values, rnd, enc, null=()):
    """InvalidArgument with the same message, which holds `text`, from both forms; every output keeps its pattern"""
    import zero_chain_amd as zk
    msgs = []
    for form in (HOST, DEVICE):
        monkeypatch.setenv(VAR, form)
        rc, left, right, st = _raw_call(lib, n, k, values, rnd, enc, null=null)
        with pytest.raises(zk.ZkError) as e:
            lib.check(rc)
        assert e.value.variant == "InvalidArgument", str(e.value)
        msgs.append(str(e.value))
        assert all((a == PATTERN).all() for a in (left, right, st))
    assert msgs[0] == msgs[1] and text in msgs[0], (text, msgs)


def test_argument_errors(lib, monkeypatch):
    rnd, enc = ec.randomness(9, 3), ec.keys(50, 6)
    values = [1, 2, 3, 4, 5, 6]
    for bad in (ec.S, (1 << 256) - 1):
        _refused(monkeypatch, lib, "randomness 1 is not a canonical Fs scalar", 3, 2, values, [rnd[0], bad, rnd[2]], enc)
    for bad in (1 << 32, -(1 << 32), (1 << 63) - 1, -(1 << 63)):
        _refused(monkeypatch, lib, "value 4 is outside (-2^32, 2^32)", 3, 2, values[:4] + [bad] + values[5:], rnd, enc)
    # a bad value goes before a bad randomness
    _refused(monkeypatch, lib, "value 5 is outside", 3, 2, values[:5] + [1 << 32], [ec.S] + rnd[1:], enc)
    for k in (0, 17):
        _refused(monkeypatch, lib, "k must be 1 .. 16", 1, k, [1] * 17, rnd[:1], ec.keys(0, 17))
    for null in ("values", "randomness", "enc_keys", "left", "right", "status"):
        _refused(monkeypatch, lib, "null argument", 3, 2, values, rnd, enc, null=(null,))


def test_no_groups_and_the_device_index(lib, monkeypatch):
    import zero_chain_amd as zk
    for form in (HOST, DEVICE):
        monkeypatch.setenv(VAR, form)
        assert lib.zk_elgamal_encrypt_dev(0, 1, None, None, None, 0, None, None, None) == 0   # n = 0 touches nothing
        rc, left, right, st = _raw_call(lib, 0, 3, [0], [0], [ec.IDENTITY])
        assert rc == 0 and all((a == PATTERN).all() for a in (left, right, st))
    assert zk.elgamal_encrypt_dev([], [], [], k=3, lib=lib) == ([], [], [])
    monkeypatch.setenv(VAR, DEVICE)
    rc, left, _, _ = _raw_call(lib, 1, 1, [1], ec.randomness(1, 1), ec.keys(0, 1), device=4096)
    with pytest.raises(zk.ZkError) as e:
        lib.check(rc)
    assert e.value.variant == "InvalidArgument" and "device index out of range" in str(e.value) and (left == PATTERN).all()


# ---------------------------------------------------------------------------------------------- wave and slice boundaries
def _ends(call):
    return (0, len(call[1]) - 1)


def test_a_second_wave_with_one_live_lane(lib, monkeypatch):
    """65 groups of k = 1 with 65 keys and 65 values: a second wave with one live lane in every lane kind"""
    call = ([1000 + i for i in range(65)], ec.randomness(10, 65), ec.keys(0, 64) + [ec.IDENTITY], 1)
    assert len(set(call[2])) == 65
    lefts, rights, statuses = check(monkeypatch, lib, call, groups=_ends(call))
    assert statuses == [0] * 65 and len(set(lefts)) == len(set(rights)) == 65


def test_sixty_six_variable_lanes(lib, monkeypatch):
    call = ec.confidential(11, 22)
    lefts, _, statuses = check(monkeypatch, lib, call, groups=_ends(call))
    assert statuses == [0] * 66 and len(set(lefts)) == 66


def test_forty_groups_share_one_ring(lib, monkeypatch):
    """12 decode lanes against 480 variable-base lanes"""
    call = ec.anonymous(12, 40, first=7, shared=True)
    assert len(set(call[2])) == 12 and len(call[2]) == 480
    lefts, rights, statuses = check(monkeypatch, lib, call, groups=_ends(call))
    assert statuses == [0] * 480 and len(set(rights)) == 40


def test_three_slices(hooks_lib, monkeypatch, request):
    """9 groups of k = 2 in slices of 4: three slices, the last partial; a refused key in the last one"""
    import zero_chain_amd as zk
    values = [(-1) ** i * (i + 1) for i in range(18)]
    enc = ec.keys(3, 17) + [sc.torsion()]
    call = (values, ec.randomness(13, 9), enc, 2)
    whole = both_forms(monkeypatch, hooks_lib, call)
    monkeypatch.setenv("ZKAMD_DEBUG_ENCRYPT_SLICE", "4")
    lefts, rights, statuses = check(monkeypatch, hooks_lib, call, groups=(0, 3, 4, 8))
    assert (lefts, rights, statuses) == whole and statuses == [0] * 17 + [3]
    if "gpu" in request.node.callspec.id:
        monkeypatch.setenv(VAR, DEVICE)
        with zk.KernelTimer(hooks_lib) as t:
            zk.elgamal_encrypt_dev(*call[:3], k=2, lib=hooks_lib)
            assert [t.get(s)[0] for s in STAGES] == [3, 3]


def test_device_memory_is_returned_and_wiped(lib, monkeypatch):
    """after a device-form call nothing that held the randomness is held, and everything released was zeroed first; the
    fixed-base table - public - stays"""
    import zero_chain_amd as zk
    monkeypatch.setenv(VAR, DEVICE)
    call = ec.confidential(2, 2)
    zk.elgamal_encrypt_dev(*call[:3], k=3, lib=lib)   # (the first kernel call of a process uploads the table, which stays)
    before = zk.memory_stats(lib=lib)
    zk.elgamal_encrypt_dev(*call[:3], k=3, lib=lib)
    after = zk.memory_stats(lib=lib)
    assert after["device_held"] == before["device_held"] and after["device_released"] == after["device_wiped"]
    assert after["device_released"] - before["device_released"] >= 2 * 32 + (6 + 2 + 6) * 128   # the randomness and the projective points


# ---------------------------------------------------------------------------------------------- gpu only
@pytest.mark.gpu
def test_round_trip_through_decrypt(gpu_lib, monkeypatch):
    """8 ciphertexts under keys made with zk_jubjub_base_mul decrypt to their values; a negative value is recovered as the
    limit-bounded x of the negated point, as zk_anonymous_scan reads it"""
    import zero_chain_amd as zk
    dks = sc.fs(14, 8)
    enc = zk.jubjub_base_mul(dks, lib=gpu_lib)
    values = [0, 1, 999999, 31337, -1, -999999, 65536, -42]
    monkeypatch.setenv(VAR, DEVICE)
    lefts, rights, statuses = zk.elgamal_encrypt_dev(values, ec.randomness(14, 8), enc, k=1, lib=gpu_lib)
    assert statuses == [0] * 8
    # -(L - dk R) = (-L) - dk (-R): the negated ciphertext decrypts to -v
    flip = lambda b: jj.write_point(sc.neg(jj.read_point(b)))
    left = [flip(l) if v < 0 else l for l, v in zip(lefts, values)]
    right = [flip(r) if v < 0 else r for r, v in zip(rights, values)]
    table = C.c_void_p()
    gpu_lib.check(gpu_lib.zk_elgamal_table_create(12, 0, C.byref(table)))
    try:
        lb, rb, kb = (np.frombuffer(b"".join(x), dtype=np.uint8).copy() for x in (left, right, [int(d).to_bytes(32, "little") for d in dks]))
        out, found = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        gpu_lib.check(gpu_lib.zk_elgamal_decrypt(table, 8, as_p(lb), as_p(rb), as_p(kb), 32, 1000000, as_p(out), as_p(found)))
        assert found.tolist() == [1] * 8 and out.tolist() == [abs(v) for v in values]
    finally:
        gpu_lib.zk_elgamal_table_free(table)


@pytest.mark.gpu
def test_the_stages_of_each_form(gpu_lib, monkeypatch):
    import zero_chain_amd as zk
    call = ec.confidential(2, 2)
    monkeypatch.setenv(VAR, DEVICE)
    with zk.KernelTimer(gpu_lib) as t:
        device = zk.elgamal_encrypt_dev(*call[:3], k=3, lib=gpu_lib)
        assert [t.get(s)[0] for s in STAGES] == [1, 1]
    monkeypatch.setenv(VAR, HOST)
    with zk.KernelTimer(gpu_lib) as t:
        host = zk.elgamal_encrypt_dev(*call[:3], k=3, lib=gpu_lib)
        assert [t.get(s)[0] for s in STAGES] == [0, 0]
    assert host == device
