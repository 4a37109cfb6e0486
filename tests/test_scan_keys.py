"""A block read with a SET of decryption keys in one call (zk_scan_keys_*, zk_confidential_scan_keys, zk_anonymous_scan_keys,
csrc/scan_keys.h): every pair (extrinsic, key) in which the extrinsic carries the key, with the 16 bytes the single-key entry writes
for that key.  Every case runs with the host form of the point work forced (ZKAMD_SCAN_HOST_MAX large) and with the kernels forced
(0) - k_keys_points, whose lanes each multiply by the scalar of their own hit: the two hit arrays must be equal byte for byte, equal
to a loop of the single-key entry over the keys, and equal to the expectation tests/scan_keys_cases.py takes from the oracle.
CPU: the x86 emulation build with 8 baby-step bits and limit 5000.  GPU: the product library with the default table."""
import ctypes as C
import os
import random

import pytest

import scan_cases as sc
import scan_keys_cases as skc
from oracle import jubjub as jj

HOST, DEVICE = str(1 << 40), "0"


def _entry(table, kind):
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    if kind == "confidential":
        return (table._lib.zk_confidential_scan_keys, table._lib.zk_confidential_scan, _lib.ConfidentialXt, zk._api._fill_confidential_xt,
                _lib.ConfidentialScanHit, _lib.ConfidentialScanResult, 2)
    return (table._lib.zk_anonymous_scan_keys, table._lib.zk_anonymous_scan, _lib.AnonymousXt, zk._api._fill_anonymous_xt, _lib.AnonymousScanHit,
            _lib.AnonymousScanResult, 12)


def hits_raw(table, kind, xts, keys, limit):
    """[(xt, key, the 16 bytes of r)] of the C entry, through the mirror's own marshalling"""
    fn, _, xt, fill, hit, _, per_xt = _entry(table, kind)
    return [(h.xt, h.key, bytes(h.r)) for h in table._scan_keys(fn, xt, fill, hit, per_xt, xts, keys, limit)]


def loop_raw(table, kind, xts, dks, limit, only=None):
    """the same list from one call of the single-key entry per key"""
    _, fn, xt, fill, _, result, _ = _entry(table, kind)
    out = []
    for k, dk in enumerate(dks):
        if only is None or k in only:
            out += [(i, k, bytes(r)) for i, r in enumerate(table._scan(fn, xt, fill, result, xts, dk, limit)) if bytes(r) != bytes(16)]
    return sorted(out)


def both_forms(monkeypatch, table, kind, xts, keys, limit):
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", HOST)
    host = hits_raw(table, kind, xts, keys, limit)
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    device = hits_raw(table, kind, xts, keys, limit)
    assert host == device, [(h, d) for h, d in zip(host, device) if h != d][:4]
    return host


def check(monkeypatch, table, kind, xts, dks, logs):
    import zero_chain_amd as zk
    want = skc.expected_hits(kind, xts, dks, logs)
    with zk.ScanKeys(dks, lib=table._lib) as keys:
        got = both_forms(monkeypatch, table, kind, xts, keys, logs.limit)
    assert got == want, ([(g[0], g[1], g[2].hex()) for g in got if g not in want][:4], [(w[0], w[1], w[2].hex()) for w in want if w not in got][:4])
    assert got == loop_raw(table, kind, xts, dks, logs.limit)
    return got


@pytest.fixture(scope="module")
def logs5000():
    return sc.Logs(5000)


@pytest.fixture(scope="module")
def emu_table(emu_lib):
    import zero_chain_amd as zk
    t = zk.ElGamalTable(8, lib=emu_lib)
    yield t
    t.close()


# ---------------------------------------------------------------------------------------------- CPU (emulation build)
def test_roles_over_a_key_set(emu_lib, emu_table, logs5000, monkeypatch):
    import zero_chain_amd as zk
    xts, _ = sc.confidential_role_cases(emu_lib, [0, 1, 255, 256, 257, 4999, 5000], 70000, 5000)
    dks = [sc.WALLET, sc.ALICE, sc.BOB]
    got = check(monkeypatch, emu_table, "confidential", xts, dks, logs5000)
    # WALLET -> ALICE and ALICE -> WALLET are hit twice, with different scalars in neighbouring lanes; WALLET -> WALLET once, role 3
    assert [(g[0], g[1], g[2][0]) for g in got[:5]] == [(0, 0, 1), (0, 1, 2), (1, 0, 2), (1, 1, 1), (2, 0, 3)]
    with zk.ScanKeys(dks, lib=emu_lib) as keys:
        res = emu_table.scan_confidential_keys(xts, keys, limit=5000)
        none = dict(refusal=None, amount_sent=None, fee=None, amount_received=None)
        assert res[0] == (0, 0, dict(none, role=zk.SCAN_SENDER, amount_sent=0, fee=3)) and res[1] == (0, 1, dict(none, role=zk.SCAN_RECIPIENT, amount_received=0))
        assert [r for r in res if r[0] == 17] == [(17, 0, dict(none, role=3, amount_sent=4999, fee=1, amount_received=4999))]
        assert [r for r in res if r[0] == 21] == [(21, 1, dict(none, role=zk.SCAN_SENDER, amount_sent=9, fee=3)), (21, 2, dict(none, role=zk.SCAN_RECIPIENT, amount_received=9))]
        assert zk.scan_confidential_keys(emu_table, xts, keys, 5000) == res
    check(monkeypatch, emu_table, "confidential", xts[:12], dks, sc.Logs(256))   # one probe per value
    # three strangers: no hit
    assert check(monkeypatch, emu_table, "confidential", xts, skc.STRANGERS, logs5000) == []


def test_edge_scalars(emu_lib, emu_table, logs5000, monkeypatch):
    """1, 2, FS_MOD - 1 (bit 251: the top window), 2^251 and 0x0777..7 (a carry into every window), each as sender and as recipient"""
    import zero_chain_amd as zk
    xts, _ = skc.edge_cases(emu_lib, [1, 255, 256, 4999, 17])
    got = check(monkeypatch, emu_table, "confidential", xts, skc.EDGE, logs5000)
    assert len(got) == 10 and all(g[2][1] == (3 if g[2][0] == sc.SENDER else 4) for g in got)
    with zk.ScanKeys(skc.EDGE, lib=emu_lib) as keys:
        g = jj.note_commitment_randomness_generator()
        assert keys.enc_keys()[:3] == [jj.write_point(g), jj.write_point(jj.add(g, g)), jj.write_point(sc.neg(g))]   # (FS_MOD - 1) G = -G


def test_lane_layout(emu_lib, emu_table, logs5000, monkeypatch):
    cycle, mixed, last, _ = skc.lane_layout_cases(emu_lib)
    got = check(monkeypatch, emu_table, "confidential", cycle, skc.CYCLE, logs5000)
    assert len(got) == 140 and all(g[2][1] == (3 if g[2][0] == sc.SENDER else 4) for g in got)
    got_mixed = check(monkeypatch, emu_table, "confidential", mixed, skc.CYCLE, logs5000)
    assert [(2 * g[0], g[1]) for g in got] == [g[:2] for g in got_mixed] and [g[2][:2] + g[2][4:] for g in got] == [g[2][:2] + g[2][4:] for g in got_mixed]
    got = check(monkeypatch, emu_table, "confidential", last, skc.CYCLE, logs5000)
    assert [(g[0], g[1], g[2][:2]) for g in got] == [(5, 3, bytes([sc.RECIPIENT, sc.FOUND_RECEIVED]))]


@pytest.mark.parametrize("matches", [1, 65])
def test_a_one_key_set_is_the_one_key_scan_in_the_device_form(emu_lib, emu_table, monkeypatch, matches):
    """The two point kernels share one lane body and differ in the multiplier (csrc/wallet_stage.h): the shared width-4 NAF of
    zk_confidential_scan's one key, the fixed windows over the lane's own scalar of a key set.  With the kernels forced, a set of
    that one key writes the 16 bytes of the one-key entry for every matching extrinsic - one multiplication lane, and a second wave of
    them."""
    import zero_chain_amd as zk
    specs = [(sc.ALICE, sc.BOB, 5, 1)] + [(sc.ALICE, sc.WALLET, 100 + j, 1) for j in range(matches)]
    xts = sc.confidential_xts(emu_lib, specs, seed=38)
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    with zk.ScanKeys([sc.WALLET], lib=emu_lib) as keys:
        got = hits_raw(emu_table, "confidential", xts, keys, 5000)
    assert [(g[0], g[1], g[2][:2], int.from_bytes(g[2][12:], "little")) for g in got] == \
        [(1 + j, 0, bytes([sc.RECIPIENT, sc.FOUND_RECEIVED]), 100 + j) for j in range(matches)]
    assert got == loop_raw(emu_table, "confidential", xts, [sc.WALLET], 5000)


def test_anonymous_rings(emu_lib, emu_table, logs5000, monkeypatch):
    import zero_chain_amd as zk
    xts, _ = skc.ring_cases(emu_lib, [1, 255, 256, 4999])
    dks = [sc.WALLET, sc.ALICE, sc.BOB]
    got = check(monkeypatch, emu_table, "anonymous", xts, dks, logs5000)
    assert [g[:2] for g in got[:5]] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2)] and all(g[0] != 8 for g in got)
    with zk.ScanKeys(dks, lib=emu_lib) as keys:
        res = emu_table.scan_anonymous_keys(xts, keys, limit=5000)
        assert res[:5] == [(0, 0, dict(members=[0], refusal=None, delta=-1)), (0, 1, dict(members=[5], refusal=None, delta=1)),
                           (0, 2, dict(members=[11], refusal=None, delta=0)), (1, 0, dict(members=[7], refusal=None, delta=-1)),
                           (1, 2, dict(members=[2, 9], refusal=None, delta=1))]
        assert zk.scan_anonymous_keys(emu_table, xts, keys, 5000) == res
    check(monkeypatch, emu_table, "anonymous", xts, dks, sc.Logs(256))
    got = check(monkeypatch, emu_table, "anonymous", xts, dks, sc.Logs(1))   # only zeros are found
    assert [g[:2] for g in got if g[2][2]] == [(0, 2), (2, 2), (4, 2), (6, 2)]
    assert check(monkeypatch, emu_table, "anonymous", xts, skc.STRANGERS, logs5000) == []


def test_refusals_per_hit(emu_lib, emu_table, logs5000, monkeypatch):
    """each hit's refusal byte follows the push order of its own role; a bad point does not disturb its neighbours, and one in an
    extrinsic no key matches is not looked at"""
    cx, ax, _ = sc.refusal_cases(emu_lib)
    got = check(monkeypatch, emu_table, "confidential", cx, [sc.WALLET, sc.ALICE], logs5000)
    by = {g[:2]: g[2] for g in got}
    # cx[6], WALLET -> WALLET: field 3 first.  cx[3], ALICE -> WALLET: the recipient's left is refused, the sender's hit is fine.
    # cx[4], WALLET -> ALICE with a bad right half: both hits are refused by it.  cx[8], ALICE -> BOB: ALICE's hit sees the right half.
    assert by[(6, 0)][2] == 3 | 1 << 6 and by[(3, 0)][2] == 4 | 3 << 6 and by[(3, 1)][2] == 0 and by[(3, 1)][1] == 3
    assert by[(4, 0)][2] == by[(4, 1)][2] == by[(8, 1)][2] == 5 | 1 << 6 and by[(5, 0)][2] == 6 | 2 << 6 and by[(5, 1)][2] == 0
    assert by[(7, 0)][2] == 0 and by[(7, 1)][2] == 3 | 3 << 6                       # the recipient's hit does not look at the sender's points
    assert [by[(k, 0)] for k in (10, 11, 12)] == [by[(k, 0)] for k in (0, 1, 2)] and by[(0, 0)][1] == sc.FOUND_RECEIVED
    # with a stranger in ALICE's place nothing of cx[8] and cx[9] is looked at
    got = check(monkeypatch, emu_table, "confidential", cx, [sc.WALLET, skc.STRANGERS[0]], logs5000)
    assert [g[0] for g in got] == [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12] and [g[2][2] for g in got] == [0, 0, 0, 4 | 3 << 6, 5 | 1 << 6, 6 | 2 << 6, 3 | 1 << 6, 0, 0, 0, 0]
    got = check(monkeypatch, emu_table, "anonymous", ax, [sc.WALLET, sc.ALICE], logs5000)
    assert [(g[0], g[1], g[2][3]) for g in got] == [(0, 0, 0), (1, 0, 19 | 3 << 6), (2, 0, 20 | 1 << 6), (3, 0, 49 | 2 << 6), (6, 0, 0)]


def test_invalid_arguments(emu_lib, emu_table, monkeypatch):
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    # the key set
    for bad, index in (([sc.WALLET, jj.FS_MOD], 1), ([(1 << 256) - 1, sc.ALICE, sc.BOB], 0)):
        with pytest.raises(zk.ZkError) as e:
            zk.ScanKeys(bad, lib=emu_lib)
        assert e.value.variant == "InvalidArgument" and "dec_key %d is not a canonical Fs scalar" % index in str(e.value)
    with pytest.raises(zk.ZkError) as e:
        zk.ScanKeys([sc.WALLET, sc.ALICE, sc.BOB, sc.ALICE], lib=emu_lib)
    assert e.value.variant == "InvalidArgument" and "dec_key 1 and dec_key 3 are equal" in str(e.value)
    with pytest.raises(zk.ZkError) as e:
        zk.ScanKeys([], lib=emu_lib)
    assert e.value.variant == "InvalidArgument"
    h = C.c_void_p()
    kb = C.create_string_buffer(b"".join(k.to_bytes(32, "little") for k in (sc.WALLET, sc.ALICE)), 64)
    for args in ((kb, 0, C.byref(h)), (None, 2, C.byref(h)), (kb, 2, None)):
        with pytest.raises(zk.ZkError) as e:
            emu_lib.check(emu_lib.zk_scan_keys_create(*args))
        assert e.value.variant == "InvalidArgument" and not h.value
    emu_lib.zk_scan_keys_free(None)
    keys = zk.ScanKeys([sc.WALLET, sc.ALICE], lib=emu_lib)
    assert len(keys) == 2 and keys.enc_keys() == zk.jubjub_base_mul([sc.WALLET, sc.ALICE], lib=emu_lib)
    assert keys.enc_keys(1) == keys.enc_keys()[1:] and keys.enc_keys(1, 1) == keys.enc_keys()[1:] and keys.enc_keys(2) == [] == keys.enc_keys(0, 0)
    out32 = C.create_string_buffer(96)
    for first, count in ((0, 3), (2, 1), (3, 0), ((1 << 64) - 1, 2)):
        with pytest.raises(zk.ZkError) as e:
            emu_lib.check(emu_lib.zk_scan_keys_get(keys._h, first, count, out32))
        assert e.value.variant == "InvalidArgument" and "outside the set" in str(e.value)
    for args in ((None, 0, 1, out32), (keys._h, 0, 1, None)):
        with pytest.raises(zk.ZkError) as e:
            emu_lib.check(emu_lib.zk_scan_keys_get(*args))
        assert "null" in str(e.value)
    # the two scans
    cx = sc.confidential_xts(emu_lib, [(sc.ALICE, sc.WALLET, 5, 1), (sc.BOB, sc.ALICE, 6, 2)])
    ax = sc.anonymous_xts(emu_lib, [skc.ring_of(emu_lib, {4: (sc.WALLET, 5), 6: (sc.ALICE, -5)})])
    carr = zk._api._xt_array(cx, _lib.ConfidentialXt, zk._api._fill_confidential_xt)
    aarr = zk._api._xt_array(ax, _lib.AnonymousXt, zk._api._fill_anonymous_xt)
    for form in (HOST, DEVICE):
        monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", form)
        for scan, xts in ((emu_table.scan_confidential_keys, cx), (emu_table.scan_anonymous_keys, ax)):
            for limit in (0, (1 << 32) + 1):
                with pytest.raises(zk.ZkError) as e:
                    scan(xts, keys, limit=limit)
                assert e.value.variant == "InvalidArgument" and "limit" in str(e.value)
            assert scan([], keys) == [] and scan(b"", keys) == []
        # the mirror on packed arrays and raw bytes
        res = emu_table.scan_confidential_keys(cx, keys, limit=5000)
        assert [r[:2] for r in res] == [(0, 0), (0, 1), (1, 1)] and res[2][2]["amount_received"] == 6
        assert emu_table.scan_confidential_keys(carr, keys, limit=5000) == res == emu_table.scan_confidential_keys(bytes(carr), keys, limit=5000)
        res = emu_table.scan_anonymous_keys(ax, keys, limit=5000)
        assert [(r[0], r[1], r[2]["delta"]) for r in res] == [(0, 0, 5), (0, 1, -5)]
        assert emu_table.scan_anonymous_keys(aarr, keys, limit=5000) == res == emu_table.scan_anonymous_keys(bytes(aarr), keys, limit=5000)
        with pytest.raises(ValueError):
            emu_table.scan_confidential_keys(bytes(carr)[:-1], keys)
        # the raw entries
        for fn, arr, n, hit, hits in ((emu_lib.zk_confidential_scan_keys, carr, 2, _lib.ConfidentialScanHit, 3), (emu_lib.zk_anonymous_scan_keys, aarr, 1, _lib.AnonymousScanHit, 2)):
            out, count = (hit * 4)(), C.c_size_t(77)
            C.memset(out, 0xa5, C.sizeof(out))
            # hits_cap one too small: the count needed, nothing written - also as a sizing call without an array
            for o, cap in ((out, hits - 1), (None, 0)):
                with pytest.raises(zk.ZkError) as e:
                    emu_lib.check(fn(emu_table._h, keys._h, n, arr, 5000, o, cap, C.byref(count)))
                assert e.value.variant == "InvalidArgument" and "hits_cap" in str(e.value) and count.value == hits
                assert bytes(out) == b"\xa5" * C.sizeof(out)
            assert fn(emu_table._h, keys._h, n, arr, 5000, out, hits, C.byref(count)) == 0 and count.value == hits
            assert bytes(out)[24 * hits:] == b"\xa5" * 24 * (4 - hits) and [(o.xt, o.key) for o in out[:hits]] == [(0, 0), (0, 1), (1, 1)][:hits]
            for args in ((None, keys._h, n, arr, 5000, out, 4, C.byref(count)), (emu_table._h, None, n, arr, 5000, out, 4, C.byref(count)),
                         (emu_table._h, keys._h, n, arr, 5000, out, 4, None), (emu_table._h, keys._h, n, None, 5000, out, 4, C.byref(count)),
                         (emu_table._h, keys._h, n, arr, 5000, None, 4, C.byref(count)), (None, None, 0, None, 5000, None, 0, None)):
                with pytest.raises(zk.ZkError) as e:
                    emu_lib.check(fn(*args))
                assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
            count.value = 77
            assert fn(emu_table._h, keys._h, 0, None, 5000, None, 0, C.byref(count)) == 0 and count.value == 0   # n == 0
    keys.close()
    keys.close()


def test_keys_points_kernel_keeps_its_tables_in_lds():
    """the code object's metadata for k_keys_points: one such kernel, no scratch memory, and LDS within k_rj_check's budget"""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources(_lib.LIB_PATH).items() if "k_keys_points" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and 0 < r["lds"] <= 36864, r


# ---------------------------------------------------------------------------------------------- GPU
BIG = [0, 1, 999999, 10 ** 6, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 32) - 1]


@pytest.fixture(scope="module")
def table(gpu_lib):
    import zero_chain_amd as zk
    t = zk.ElGamalTable(lib=gpu_lib)
    yield t
    t.close()


@pytest.mark.gpu
def test_gpu_roles_edge_scalars_and_refusals(gpu_lib, table, monkeypatch):
    xts, cand = sc.confidential_role_cases(gpu_lib, BIG, (1 << 31) + 5, 10 ** 6)
    ex, cand1 = skc.edge_cases(gpu_lib, BIG[3:])
    cx, ax, cand2 = sc.refusal_cases(gpu_lib)
    for limit in (10 ** 6, 1 << 32):
        logs = sc.Logs(limit, cand + cand1 + cand2)
        got = check(monkeypatch, table, "confidential", xts, [sc.WALLET, sc.ALICE, sc.BOB], logs)
        # WALLET to itself with 2^32 - 1: all three values at 2^32, only the fee at 10^6
        assert [g[2][:2] for g in got if g[0] == 23] == [bytes([3, 7 if limit > 10 ** 6 else sc.FOUND_FEE])]
        assert check(monkeypatch, table, "confidential", xts, skc.STRANGERS, logs) == []
        assert len(check(monkeypatch, table, "confidential", ex, skc.EDGE, logs)) == 10
        got = check(monkeypatch, table, "confidential", cx, [sc.WALLET, sc.ALICE], logs)
        assert [g[2][2] for g in got if g[1] == 0] == [0, 0, 0, 4 | 3 << 6, 5 | 1 << 6, 6 | 2 << 6, 3 | 1 << 6, 0, 0, 0, 0]
        got = check(monkeypatch, table, "anonymous", ax, [sc.WALLET, sc.ALICE], logs)
        assert [(g[0], g[2][3]) for g in got] == [(0, 0), (1, 19 | 3 << 6), (2, 20 | 1 << 6), (3, 49 | 2 << 6), (6, 0)]


@pytest.mark.gpu
def test_gpu_lane_layout(gpu_lib, table, monkeypatch):
    cycle, mixed, last, _ = skc.lane_layout_cases(gpu_lib)
    logs = sc.Logs(5000)
    assert len(check(monkeypatch, table, "confidential", cycle, skc.CYCLE, logs)) == 140
    assert len(check(monkeypatch, table, "confidential", mixed, skc.CYCLE, logs)) == 140
    assert len(check(monkeypatch, table, "confidential", last, skc.CYCLE, logs)) == 1


@pytest.mark.gpu
def test_gpu_anonymous_rings(gpu_lib, table, monkeypatch):
    xts, cand = skc.ring_cases(gpu_lib, BIG[1:])
    for limit in (10 ** 6, 1 << 32):
        got = check(monkeypatch, table, "anonymous", xts, [sc.WALLET, sc.ALICE, sc.BOB], sc.Logs(limit, cand))
        assert len(got) == 5 * len(BIG[1:])


@pytest.mark.gpu
def test_gpu_random_block_of_forty_keys(gpu_lib, table, monkeypatch):
    """300 confidential and 300 anonymous extrinsics over 40 keys and 20 strangers: the expectation is the plaintext each was built
    from (the oracle holds the small cases above); five of the keys are also read one by one with the single-key entries"""
    import zero_chain_amd as zk
    rng = random.Random(41)
    amount = lambda: rng.randrange(10 ** 6) if rng.randrange(3) else rng.randrange(10 ** 6, 1 << 32)
    dks, cx, ax, hits_c, hits_a = skc.random_block(gpu_lib, rng, 40, 20, 300, amount)
    five = (0, 7, 19, 20, 39)
    with zk.ScanKeys(dks, lib=gpu_lib) as keys:
        for limit, n in ((10 ** 6, 300), (1 << 32, 64)):
            got = both_forms(monkeypatch, table, "confidential", cx[:n], keys, limit)
            assert got == [(i, k, skc.confidential_bytes(role, values, limit)) for i, k, role, values in hits_c if i < n]
            assert [g for g in got if g[1] in five] == loop_raw(table, "confidential", cx[:n], dks, limit, five)
            got = both_forms(monkeypatch, table, "anonymous", ax[:n], keys, limit)
            assert got == [(i, k, skc.anonymous_bytes(members, v, limit)) for i, k, members, v in hits_a if i < n]
            assert [g for g in got if g[1] in five] == loop_raw(table, "anonymous", ax[:n], dks, limit, five)
    assert len(hits_c) > 300 and len(hits_a) > 2000


@pytest.mark.gpu
def test_gpu_scan_keys_memory_is_returned_and_wiped(gpu_lib, monkeypatch):
    import zero_chain_amd as zk
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    xts = sc.confidential_xts(gpu_lib, [(sc.WALLET, sc.WALLET, 5, 1), (sc.ALICE, sc.WALLET, 123456789, 2)])
    before = zk.memory_stats(lib=gpu_lib)
    with zk.ScanKeys([sc.WALLET, sc.ALICE], lib=gpu_lib) as keys:
        assert zk.memory_stats(lib=gpu_lib)["device_held"] == before["device_held"]   # the key set binds no device
        with zk.ElGamalTable(lib=gpu_lib) as t:
            built = zk.memory_stats(lib=gpu_lib)["device_held"]
            res = t.scan_confidential_keys(xts, keys, limit=1 << 32)
            assert [(r[0], r[1], r[2]["amount_received"], r[2]["amount_sent"]) for r in res] == [(0, 0, 5, 5), (1, 0, 123456789, None), (1, 1, None, 123456789)]
            assert zk.memory_stats(lib=gpu_lib)["device_held"] > built   # the stage's buffers stay with the table
    after = zk.memory_stats(lib=gpu_lib)
    assert after["device_held"] == before["device_held"]
    assert after["device_released"] == after["device_wiped"] > before["device_released"]
