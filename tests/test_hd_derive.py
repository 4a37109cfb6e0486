"""Hierarchical key derivation in one call (zk_hd_master, zk_hd_xpgk_from_xsk, zk_hd_derive, zk_scan_keys_create_hd,
zk_jubjub_base_mul_dev; csrc/hd_keys.h) against the Python model of tests/hd_cases.py.

Every case runs on the x86 emulation build and, marked gpu, on the product library, each time with the host form of the point work
forced (ZKAMD_HD_HOST_MAX large) and with the kernel forced (0): the two outputs must be equal byte for byte and equal to the model.
The model answers to the reference by the reference's own three invariants (derive/mod.rs:267-319), asserted here on the library's
outputs; by the one pin the reference holds for the account step (the encryption key of the seed "Alice" + 27 spaces); and by byte
pins recorded from the model (hd_cases.PIN_*, regression anchors only).  Model-checked children stay at or below 70 per test; larger
counts compare the two forms alone.  No test runs more than 130 lanes of a kernel."""
import ctypes as C
import os
import random

import pytest

import hd_cases as hc
import scan_cases as sc
from oracle import gen_proof as gp
from oracle import jubjub as jj

HOST, DEVICE = str(1 << 40), "0"
ALICE_SEED = b"Alice" + b" " * 27                                               # modules/encrypted-balances/src/lib.rs:381
ALICE_ENC_KEY = "fd0c0c0183770c99559bf64df4fe23f77ced9b8b4d02826a282bcd125117dcc2"   # :443 pkd_addr_alice
OTHER_SEED = bytes(range(100, 140))
SMALL_ORDER = (jj.R - 1).to_bytes(32, "little")                                  # (0, -1): on the curve, of order 2


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "gpu_lib")


_model = {}   # (kind, xkey, index) -> (xkey, dec_key, enc_key) of that child: computed once, shared by the tests


def model(kind, xkey, indices):
    missing = [i for i in dict.fromkeys(indices) if (kind, xkey, i) not in _model]
    if missing:
        for i, x, d, e in zip(missing, *hc.derive(kind, xkey, missing)):
            _model[(kind, xkey, i)] = (x, d, e)
    rows = [_model[(kind, xkey, i)] for i in indices]
    return tuple([r[k] for r in rows] for k in range(3))


def both_forms(monkeypatch, lib, xkey, indices, kind, **kw):
    import zero_chain_amd as zk
    monkeypatch.setenv("ZKAMD_HD_HOST_MAX", HOST)
    host = zk.hd_derive(xkey, indices, kind=kind, lib=lib, **kw)
    monkeypatch.setenv("ZKAMD_HD_HOST_MAX", DEVICE)
    device = zk.hd_derive(xkey, indices, kind=kind, lib=lib, **kw)
    assert host == device
    return host


def check(monkeypatch, lib, xkey, indices, kind):
    got = both_forms(monkeypatch, lib, xkey, indices, kind)
    want = model(kind, xkey, indices)
    assert got == want
    return got


def test_master_children_and_their_accounts_are_the_pinned_bytes(lib, monkeypatch):
    """(c) the regression anchors: recorded from the model, not from the reference"""
    import zero_chain_amd as zk
    m = zk.hd_master(hc.PIN_SEED, lib=lib)
    assert m == hc.PIN_MASTER == hc.master(hc.PIN_SEED) and len(m) == zk.HD_XKEY_BYTES
    assert zk.hd_master(b"", lib=lib) == hc.master(b"") and zk.hd_master(OTHER_SEED, lib=lib) == hc.master(OTHER_SEED)
    assert zk.hd_xpgk(m, lib=lib) == hc.xpgk_of(m)
    got = check(monkeypatch, lib, m, hc.PIN_INDICES, zk.HD_XSK)
    assert got == (hc.PIN_CHILDREN, hc.PIN_DEC_KEYS, hc.PIN_ENC_KEYS)


def test_the_references_three_invariants_hold_on_the_librarys_outputs(lib, monkeypatch):
    """(a) derive/mod.rs:267-319, on what the LIBRARY writes: the xpgk of the xsk child 3 is the child 3 of the xpgk; a hardened child
    is refused on the xpgk route; the same equality for h3 / n5; what the library writes, it reads back as the same key"""
    import zero_chain_amd as zk
    for seed in (hc.PIN_SEED, OTHER_SEED):
        xsk_m = zk.hd_master(seed, lib=lib)
        xpgk_m = zk.hd_xpgk(xsk_m, lib=lib)
        for form in (HOST, DEVICE):
            monkeypatch.setenv("ZKAMD_HD_HOST_MAX", form)
            # derive_nonhardened_child
            (xsk_3,), dk_s, enc_s = zk.hd_derive(xsk_m, [3], kind=zk.HD_XSK, lib=lib)
            (xpgk_3,), dk_p, enc_p = zk.hd_derive(xpgk_m, [3], kind=zk.HD_XPGK, lib=lib)
            assert zk.hd_xpgk(xsk_3, lib=lib) == xpgk_3 and dk_s == dk_p and enc_s == enc_p
            # derive_hardened_child
            h3 = hc.HARDENED + 3
            (xsk_h3,), _, _ = zk.hd_derive(xsk_m, [h3], kind=zk.HD_XSK, lib=lib)
            with pytest.raises(zk.ZkError) as e:
                zk.hd_derive(xpgk_m, [h3], kind=zk.HD_XPGK, lib=lib)
            assert e.value.variant == "InvalidArgument" and "index 0 (%d) is hardened" % h3 in str(e.value)
            xpgk_h3 = zk.hd_xpgk(xsk_h3, lib=lib)
            (xsk_h3_n5,), dk_s, enc_s = zk.hd_derive(xsk_h3, [5], kind=zk.HD_XSK, lib=lib)
            (xpgk_h3_n5,), dk_p, enc_p = zk.hd_derive(xpgk_h3, [5], kind=zk.HD_XPGK, lib=lib)
            assert zk.hd_xpgk(xsk_h3_n5, lib=lib) == xpgk_h3_n5 and dk_s == dk_p and enc_s == enc_p
            # read_write: the 73 bytes the library wrote are a parent it reads as the model reads them (every field is used by a
            # child: depth, chain code, key; tag and index pass through zk_hd_xpgk_from_xsk unchanged)
            assert xpgk_h3[:41] == xsk_h3[:41] and xsk_h3[0] == 1 and xsk_h3[5:9] == h3.to_bytes(4, "little")
            assert (xsk_h3_n5,) == tuple(model(zk.HD_XSK, xsk_h3, [5])[0]) and (xpgk_h3_n5,) == tuple(model(zk.HD_XPGK, xpgk_h3, [5])[0])
            assert xsk_h3_n5[0] == 2 and xsk_h3_n5[1:5] == hc.tag_of(xpgk_h3[41:])


def test_the_account_step_is_the_one_the_references_pin_checks(lib, monkeypatch):
    """(b) The reference's one pin for the account step: the encryption key of the seed "Alice" + 27 spaces (fd0c0c01...dcc2).
    A parent whose child HAS Alice's spending key cannot be constructed: f is a hash of the parent's own key (its sk bytes for a
    hardened index, its pgk for any other), so sk_parent = sk_Alice - f(sk_parent) is a fixed point of BLAKE2b, and the same circle
    closes on the xpgk route.  What can be had: the model's account step is the function the pin checks (gen_proof.derive); the
    library's account step equals it on a child of either route, in both forms; and the library's multiplier - the kernel behind
    both multiplications of a child - reaches the pinned bytes themselves from Alice's keys."""
    import zero_chain_amd as zk
    sk_alice = gp.spending_key_from_seed(ALICE_SEED)
    pgk_alice, dk_alice, enc_alice = gp.derive(sk_alice)
    assert jj.write_point(enc_alice).hex() == ALICE_ENC_KEY and hc.account_of(jj.write_point(pgk_alice)) == (dk_alice, jj.write_point(enc_alice))
    assert zk.jubjub_base_mul_dev([sk_alice, dk_alice], lib=lib) == [jj.write_point(pgk_alice), bytes.fromhex(ALICE_ENC_KEY)]
    # a one-child case on each route: the child's spending key is sk_parent + f, and its account is gen_proof.derive's of that key
    parent = hc.pack(3, b"\x01\x02\x03\x04", 9, bytes(range(32, 64)), sk_alice.to_bytes(32, "little"))
    account = {}
    for index in (7, hc.HARDENED + 7):
        f, _ = hc.f_and_chain(parent[9:41], parent[41:], jj.write_point(pgk_alice), index)
        (child,), (dk,), (enc,) = both_forms(monkeypatch, lib, parent, [index], zk.HD_XSK)
        child_sk = int.from_bytes(child[41:], "little")
        assert child_sk == (sk_alice + f) % jj.FS_MOD
        _, dk_want, enc_want = gp.derive(child_sk)
        assert (dk, enc) == (dk_want, jj.write_point(enc_want))
        account[index] = (hc.xpgk_of(child), dk, enc)
    (child,), (dk,), (enc,) = both_forms(monkeypatch, lib, hc.xpgk_of(parent), [7], zk.HD_XPGK)
    assert (child, dk, enc) == account[7]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_children_in_order_on_both_routes(lib, monkeypatch, n):
    """one lane, a wave less one, a full wave, a wave and one: the children 0 .. n - 1 of one parent (the model computes 65 per route, once)"""
    import zero_chain_amd as zk
    xsk = hc.master(OTHER_SEED)
    check(monkeypatch, lib, xsk, list(range(n)), zk.HD_XSK)
    check(monkeypatch, lib, hc.xpgk_of(xsk), list(range(n)), zk.HD_XPGK)


def test_index_mixes(lib, monkeypatch):
    import zero_chain_amd as zk
    xsk = hc.master(OTHER_SEED)
    xpgk = hc.xpgk_of(xsk)
    top = hc.HARDENED - 1
    check(monkeypatch, lib, xpgk, [0, top, 0, 5, 5, top, 64, 3, 2, 1, 0], zk.HD_XPGK)   # the ends, repeated, descending
    check(monkeypatch, lib, xsk, [hc.HARDENED, (1 << 32) - 1, 0, top, hc.HARDENED, 9, 8, 7], zk.HD_XSK)
    got = check(monkeypatch, lib, xsk, [4, 4], zk.HD_XSK)
    assert got[0][0] == got[0][1] and got[1][0] == got[1][1]


def test_two_waves_and_a_tail_in_both_forms(lib, monkeypatch):
    """130 children: host form against device form (the model holds the first 65)"""
    import zero_chain_amd as zk
    xpgk = hc.xpgk_of(hc.master(OTHER_SEED))
    indices = list(range(129, -1, -1))
    got = both_forms(monkeypatch, lib, xpgk, indices, zk.HD_XPGK)
    want = model(zk.HD_XPGK, xpgk, list(range(64, -1, -1)))
    assert tuple(g[65:] for g in got) == want and len(set(got[1])) == 130
    monkeypatch.setenv("ZKAMD_HD_STAGE_TABLE", "1")   # the kernel's other way to read its table
    monkeypatch.setenv("ZKAMD_HD_HOST_MAX", DEVICE)
    assert zk.hd_derive(xpgk, indices, kind=zk.HD_XPGK, lib=lib) == got
    sk = [k + 1 for k in got[1][:70]]
    assert zk.jubjub_base_mul_dev(sk, lib=lib) == zk.jubjub_base_mul(sk, lib=lib)


def test_each_output_may_be_null(lib, monkeypatch):
    import zero_chain_amd as zk
    xsk = hc.master(OTHER_SEED)
    names = ("xkeys", "dec_keys", "enc_keys")
    for kind, xkey in ((zk.HD_XSK, xsk), (zk.HD_XPGK, hc.xpgk_of(xsk))):
        full = check(monkeypatch, lib, xkey, [2, 0, 1], kind)
        for drop in range(3):
            want = tuple(n for k, n in enumerate(names) if k != drop)
            got = both_forms(monkeypatch, lib, xkey, [2, 0, 1], kind, want=want)
            assert got == tuple(None if k == drop else full[k] for k in range(3))
        assert both_forms(monkeypatch, lib, xkey, [2, 0, 1], kind, want=()) == (None, None, None)


def test_chaining(lib, monkeypatch):
    """master -> 2^31 + 3 -> 5 on the xsk route against xpgk_from_xsk(master -> 2^31 + 3) -> 5"""
    import zero_chain_amd as zk
    m = zk.hd_master(hc.PIN_SEED, lib=lib)
    (h3,), _, _ = check(monkeypatch, lib, m, [hc.HARDENED + 3], zk.HD_XSK)
    (by_sk,), dk_s, enc_s = check(monkeypatch, lib, h3, [5], zk.HD_XSK)
    (by_pgk,), dk_p, enc_p = check(monkeypatch, lib, zk.hd_xpgk(h3, lib=lib), [5], zk.HD_XPGK)
    assert zk.hd_xpgk(by_sk, lib=lib) == by_pgk and dk_s == dk_p and enc_s == enc_p and by_sk[0] == by_pgk[0] == 2


def _raw_derive(lib, kind, xkey, indices, null=()):
    """zk_hd_derive through ctypes with outputs filled with 0xa5: (status, the three buffers' bytes)"""
    n = len(indices)
    ib = (C.c_uint32 * max(n, 1))(*indices)
    outs = [C.create_string_buffer(b"\xa5" * (w * max(n, 1)), w * max(n, 1)) for w in (73, 32, 32)]
    args = [None if k in null else o for k, o in enumerate(outs)]
    xb = C.create_string_buffer(bytes(xkey), 73) if xkey is not None else None
    st = lib.zk_hd_derive(kind, xb, ib if indices is not None else None, n, 0, *args)
    return st, [o.raw for o in outs]


def test_refusals_write_nothing(lib, monkeypatch):
    import zero_chain_amd as zk
    xsk = hc.master(OTHER_SEED)
    xpgk = hc.xpgk_of(xsk)
    head = xsk[:41]
    bad_y = sc.off_curve()
    cases = [
        (zk.HD_XPGK, xpgk, [hc.HARDENED, 1, 2], "index 0 (%d) is hardened" % hc.HARDENED),
        (zk.HD_XPGK, xpgk, [1, 2, (1 << 32) - 1], "index 2 (%d) is hardened" % ((1 << 32) - 1)),
        (zk.HD_XPGK, xpgk, [1, hc.HARDENED + 1, hc.HARDENED + 2], "index 1 "),                      # the FIRST such position
        (zk.HD_XSK, b"\xff" + xsk[1:], [0], "depth is 255"),
        (zk.HD_XPGK, b"\xff" + xpgk[1:], [0], "depth is 255"),
        (zk.HD_XSK, head + jj.FS_MOD.to_bytes(32, "little"), [0], "not a canonical Fs scalar"),
        (zk.HD_XSK, head + b"\xff" * 32, [hc.HARDENED], "not a canonical Fs scalar"),
        (zk.HD_XPGK, head + bad_y, [0], "is not a Jubjub point"),
        (zk.HD_XPGK, head + sc.NOT_A_POINT, [0], "is not a Jubjub point"),
        (zk.HD_XPGK, head + SMALL_ORDER, [0], "not in the prime-order subgroup"),
        (zk.HD_XPGK, head + sc.torsion(), [0], "not in the prime-order subgroup"),
        (2, xsk, [0], "kind"),
    ]
    for form in (HOST, DEVICE):
        monkeypatch.setenv("ZKAMD_HD_HOST_MAX", form)
        for kind, xkey, indices, text in cases:
            st, outs = _raw_derive(lib, kind, xkey, indices)
            with pytest.raises(zk.ZkError) as e:
                lib.check(st)
            assert e.value.variant == "InvalidArgument" and text in str(e.value), (text, str(e.value))
            assert all(o == b"\xa5" * len(o) for o in outs)
            with pytest.raises(zk.ZkError) as e:
                zk.ScanKeys.from_hd(xkey, indices, kind=kind, lib=lib)
            assert e.value.variant == "InvalidArgument" and text in str(e.value)
        # n == 0 touches nothing, whatever else is passed; NULL where something is needed is refused
        st, outs = _raw_derive(lib, zk.HD_XPGK, None, [])
        assert st == 0 and all(o == b"\xa5" * len(o) for o in outs)
        assert zk.hd_derive(xsk, [], lib=lib) == ([], [], [])
        st, outs = _raw_derive(lib, zk.HD_XSK, None, [1])
        with pytest.raises(zk.ZkError) as e:
            lib.check(st)
        assert "null" in str(e.value) and all(o == b"\xa5" * len(o) for o in outs)
        with pytest.raises(zk.ZkError) as e:
            lib.check(lib.zk_hd_derive(zk.HD_XSK, C.create_string_buffer(xsk, 73), None, 1, 0, None, None, None))
        assert "null" in str(e.value)
    # the other entries
    out = C.create_string_buffer(73)
    for args in ((None, 4, out), (b"seed", 4, None)):
        with pytest.raises(zk.ZkError) as e:
            lib.check(lib.zk_hd_master(*args))
        assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
    for args in ((None, out), (C.create_string_buffer(xsk, 73), None)):
        with pytest.raises(zk.ZkError) as e:
            lib.check(lib.zk_hd_xpgk_from_xsk(*args))
        assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
    with pytest.raises(zk.ZkError) as e:
        zk.hd_xpgk(head + jj.FS_MOD.to_bytes(32, "little"), lib=lib)
    assert e.value.variant == "InvalidArgument" and "not a canonical Fs scalar" in str(e.value)
    # a parent of depth 254 still has children, of depth 255
    (child,), _, _ = check(monkeypatch, lib, b"\xfe" + xpgk[1:], [1], zk.HD_XPGK)
    assert child[0] == 255


# ---------------------------------------------------------------------------------------------- the multiplier, with chosen digits
CARRY = sum(32 << (6 * w) for w in range(42))                            # windows 100000: digits -32, -31 x 41, and +1 in window 42
SWING = sum((32 if w % 2 == 0 else 31) << (6 * w) for w in range(42))     # windows 100000 011111 ..: digits -32, +32, -32 .. +32, 0
EDGE_SCALARS = [0, 1, 2, 31, 32, 33, (1 << 6) - 1, 1 << 251, jj.FS_MOD - 1, CARRY, SWING, (1 << 251) - 1]
assert hc.booth_digits(CARRY) == [-32] + [-31] * 41 + [1] and hc.booth_digits(SWING) == [-32, 32] * 21 + [0]
assert all(k < jj.FS_MOD for k in EDGE_SCALARS)
_mul = {}


def g_times(k):
    if k not in _mul:
        _mul[k] = jj.mul(hc.G, k)
    return _mul[k]


def test_base_mul_dev_against_the_host_entry_and_integers(lib):
    """the only cases that put CHOSEN digits through the kernels' fixed_mul"""
    import zero_chain_amd as zk
    rnd = sc.fs(161, 64)
    scalars = EDGE_SCALARS + rnd
    got = zk.jubjub_base_mul_dev(scalars, lib=lib)
    assert got == zk.jubjub_base_mul(scalars, lib=lib)
    assert got[:len(EDGE_SCALARS) + 4] == [jj.write_point(g_times(k)) for k in scalars[:len(EDGE_SCALARS) + 4]]
    assert got[0] == jj.write_point(jj.ZERO) and got[8] == jj.write_point(sc.neg(hc.G))
    assert zk.jubjub_base_mul_dev([], lib=lib) == []
    # addends: the neutral element, G, -[k]G (the sum is the neutral element), a small-order point (accepted: no subgroup test),
    # the torsion point of the scans' cases, and the two kinds of encodings Point::read refuses
    ks = EDGE_SCALARS + rnd[:4]
    good = []
    for k in ks:
        good += [(k, jj.ZERO), (k, hc.G), (k, sc.neg(g_times(k))), (k, (0, jj.R - 1)), (k, jj.read_point(sc.torsion()))]
    bad = [(ks[3], sc.NOT_A_POINT, sc.NOT_IN_FIELD), (ks[9], sc.off_curve(), sc.NOT_ON_CURVE), (0, sc.NOT_A_POINT, sc.NOT_IN_FIELD)]
    scalars = [k for k, _ in good] + [b[0] for b in bad]
    addends = [jj.write_point(p) for _, p in good] + [b[1] for b in bad]
    pts, status = zk.jubjub_base_mul_dev(scalars, addends, lib=lib)
    assert status == [0] * len(good) + [b[2] for b in bad]
    assert pts == [jj.write_point(jj.add(g_times(k), p)) for k, p in good] + [bytes(32)] * len(bad)
    assert pts[2] == pts[7] == jj.write_point(jj.ZERO)
    # a refused neighbour changes nothing around it
    assert zk.jubjub_base_mul_dev([5, 6, 7], [jj.write_point(hc.G), sc.NOT_A_POINT, jj.write_point(hc.G)], lib=lib) == \
        ([jj.write_point(g_times(6)), bytes(32), jj.write_point(g_times(8))], [0, sc.NOT_IN_FIELD, 0])
    # the scalar rule of zk_jubjub_base_mul, and the arguments
    for bad_scalars, index in (([1, jj.FS_MOD], 1), ([(1 << 256) - 1, 2, 3], 0)):
        with pytest.raises(zk.ZkError) as e:
            zk.jubjub_base_mul_dev(bad_scalars, lib=lib)
        assert e.value.variant == "InvalidArgument" and "scalar %d is not a canonical Fs scalar" % index in str(e.value)
    buf, out = C.create_string_buffer(32), C.create_string_buffer(b"\xa5" * 32, 32)
    for args in ((None, None, 1, 0, out, None), (buf, None, 1, 0, None, None), (buf, buf, 1, 0, out, None)):
        with pytest.raises(zk.ZkError) as e:
            lib.check(lib.zk_jubjub_base_mul_dev(*args))
        assert e.value.variant == "InvalidArgument" and "null" in str(e.value) and out.raw == b"\xa5" * 32
    assert lib.zk_jubjub_base_mul_dev(None, None, 0, 0, None, None) == 0


# ---------------------------------------------------------------------------------------------- the key set of the children
def test_scan_keys_from_hd(lib, monkeypatch):
    import zero_chain_amd as zk
    xpgk = hc.xpgk_of(hc.master(OTHER_SEED))
    indices = [3, 0, 64, 1]
    _, dks, encs = model(zk.HD_XPGK, xpgk, indices)
    xts = sc.confidential_xts(lib, [(dks[0], dks[3], 5, 1), (sc.ALICE, dks[1], 77, 2), (sc.ALICE, sc.BOB, 9, 1), (dks[2], dks[2], 4999, 0)], seed=51)
    with zk.ElGamalTable(8, lib=lib) as table, zk.ScanKeys(dks, lib=lib) as plain:
        want = table.scan_confidential_keys(xts, plain, limit=5000)
        assert [w[:2] for w in want] == [(0, 0), (0, 3), (1, 1), (3, 2)] and want[2][2]["amount_received"] == 77
        for form in (HOST, DEVICE):
            monkeypatch.setenv("ZKAMD_HD_HOST_MAX", form)
            with zk.ScanKeys.from_hd(xpgk, indices, kind=zk.HD_XPGK, lib=lib) as keys:
                assert len(keys) == 4 and keys.enc_keys() == encs == plain.enc_keys() == zk.hd_derive(xpgk, indices, kind=zk.HD_XPGK, lib=lib)[2]
                assert table.scan_confidential_keys(xts, keys, limit=5000) == want
            # the xsk route gives the same set for the same non-hardened children
            with zk.ScanKeys.from_hd(hc.master(OTHER_SEED), indices, kind=zk.HD_XSK, lib=lib) as keys:
                assert keys.enc_keys() == encs
            with pytest.raises(zk.ZkError) as e:
                zk.ScanKeys.from_hd(xpgk, [3, 0, 64, 0, 1], kind=zk.HD_XPGK, lib=lib)
            assert e.value.variant == "InvalidArgument" and "dec_key 1 and dec_key 3 are equal" in str(e.value)
            with pytest.raises(zk.ZkError) as e:
                zk.ScanKeys.from_hd(xpgk, [], kind=zk.HD_XPGK, lib=lib)
            assert e.value.variant == "InvalidArgument"
    h = C.c_void_p(5)
    xb, ib = C.create_string_buffer(xpgk, 73), (C.c_uint32 * 2)(1, 2)
    for args in ((1, None, ib, 2, 0, C.byref(h)), (1, xb, None, 2, 0, C.byref(h)), (1, xb, ib, 2, 0, None)):
        with pytest.raises(zk.ZkError) as e:
            lib.check(lib.zk_scan_keys_create_hd(*args))
        assert e.value.variant == "InvalidArgument" and "null" in str(e.value) and (args[5] is None or not h.value)


def test_key_derived_device_memory_is_returned_and_wiped(lib, monkeypatch):
    """after a device-form call nothing key-derived is held, and everything released was zeroed first; the table - public - stays"""
    import zero_chain_amd as zk
    xpgk = hc.xpgk_of(hc.master(OTHER_SEED))
    monkeypatch.setenv("ZKAMD_HD_HOST_MAX", DEVICE)
    zk.hd_derive(xpgk, [0], kind=zk.HD_XPGK, lib=lib)   # (the first kernel call of a process uploads the table: 132 096 bytes that stay)
    before = zk.memory_stats(lib=lib)
    got = zk.hd_derive(xpgk, list(range(65)), kind=zk.HD_XPGK, lib=lib)
    assert got == model(zk.HD_XPGK, xpgk, list(range(65)))
    with zk.ScanKeys.from_hd(xpgk, [1, 2, 3], kind=zk.HD_XPGK, lib=lib):
        zk.jubjub_base_mul_dev([1, 2, 3], [jj.write_point(hc.G)] * 3, lib=lib)
    with pytest.raises(zk.ZkError):
        zk.hd_derive(xpgk, [1, hc.HARDENED], kind=zk.HD_XPGK, lib=lib)
    after = zk.memory_stats(lib=lib)
    assert after["device_held"] == before["device_held"]
    assert after["device_released"] == after["device_wiped"] and after["device_released"] - before["device_released"] >= 65 * (32 + 96)


def test_the_kernels_keep_their_tables_in_lds():
    """the code object's metadata: both forms of both kernels, no scratch memory, LDS 17 slots (+ one staged window)"""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources(_lib.LIB_PATH).items() if "k_hd_children" in n or "k_base_mul" in n}
    assert len(res) == 4, sorted(res)
    assert all(r["scratch"] == 0 for r in res.values()), res
    assert sorted(r["lds"] for r in res.values()) == [17 * 32 * 64] * 2 + [17 * 32 * 64 + 32 * 96] * 2, res
