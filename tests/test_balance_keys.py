"""The balances of the accounts of a key set in one call (zk_balance_keys, csrc/balance_keys.h): for every account whose enc_key
is a key of the set, EncryptedBalance (+ PendingTransfer where ZK_BLOCK_ROLLOVER_DUE is set), the 64 bytes of the total and its
plaintext.  Every case runs with the host form of the point work forced (ZKAMD_SCAN_HOST_MAX large) and with the kernels forced (0)
- k_keys_points and k_balance_combine: the two hit arrays must be equal byte for byte, equal to the expectation
tests/balance_cases.py takes from the oracle, and agree with the route a caller had before: enc_total with zk_elgamal_add of the
two ciphertexts, value / found with zk_elgamal_decrypt of that total.
CPU: the x86 emulation build with 8 baby-step bits and limit 5000.  GPU: the product library with the default table."""
import ctypes as C
import os
import random

import pytest

import balance_cases as bc
import scan_cases as sc
import scan_keys_cases as skc

HOST, DEVICE = str(1 << 40), "0"
SMALL = [0, 1, 255, 256, 257, 4999, 5000]


def hits_raw(table, accs, keys, limit):
    """the 80 bytes of every hit of the C entry, the array sized by the account count"""
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    arr = zk._api._account_array(accs)
    out, count = (_lib.BalanceHit * max(len(arr), 1))(), C.c_size_t(0)
    table._lib.check(table._lib.zk_balance_keys(table._h, keys._h, len(arr), arr if len(arr) else None, int(limit), out, len(arr), C.byref(count)))
    return [bytes(h) for h in out[:count.value]]


def both_forms(monkeypatch, table, accs, keys, limit):
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", HOST)
    host = hits_raw(table, accs, keys, limit)
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    device = hits_raw(table, accs, keys, limit)
    assert host == device, [(h.hex(), d.hex()) for h, d in zip(host, device) if h != d][:4]
    return host


def two_calls(table, accs, dks, hits, limit):
    """zk_elgamal_add of the two ciphertexts (Ciphertext::zero() in the pending's place where the account is not due), then
    zk_elgamal_decrypt of the sum with the hit's key - for the hits without a refusal: those two entries fail a whole call on one"""
    import zero_chain_amd as zk
    fine = [bc.HIT.unpack(h) for h in hits if not bc.HIT.unpack(h)[3]]
    if not fine:
        return
    bal = [accs[h[0]]["balance"] for h in fine]
    pen = [accs[h[0]]["pending"] if h[4] else bc.ZERO_CT for h in fine]
    left, right = zk.elgamal_add([c[0] for c in bal], [c[1] for c in bal], [c[0] for c in pen], [c[1] for c in pen], lib=table._lib)
    assert [l + r for l, r in zip(left, right)] == [h[7] for h in fine]
    values = table.decrypt(left, right, [dks[h[1]] for h in fine], limit=limit)
    assert values == [h[6] if h[2] else None for h in fine]


def check(monkeypatch, table, accs, dks, logs):
    import zero_chain_amd as zk
    want = bc.expected_hits(accs, dks, logs)
    with zk.ScanKeys(dks, lib=table._lib) as keys:
        got = both_forms(monkeypatch, table, accs, keys, logs.limit)
    assert got == want, ([g.hex() for g in got if g not in want][:3], [w.hex() for w in want if w not in got][:3])
    two_calls(table, accs, dks, got, logs.limit)
    return [bc.HIT.unpack(g) for g in got]


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
def test_values_and_limits(emu_lib, emu_table, logs5000, monkeypatch):
    accs, cand = bc.value_cases(emu_lib, SMALL, 5000)
    dks = [sc.ALICE, sc.WALLET]
    got = check(monkeypatch, emu_table, accs, dks, logs5000)
    assert len(got) == len(accs) and all(g[1] == 1 and g[4] == 1 for g in got[:-1])
    # 4999 + 1: not found below 5000 with the pending, found with the bit clear - and with the limit one higher
    assert got[-2][2:7] == (0, 0, 1, 0, 0) and got[-1][2:7] == (1, 0, 0, 0, 4999) and got[-2][7] != got[-1][7]
    assert [g[6] for g in got[:4]] == [0, 256, 2, 258] and all(g[2] == 1 for g in got[:4])
    got = check(monkeypatch, emu_table, accs, dks, sc.Logs(5001, cand))
    assert got[-2][2:7] == (1, 0, 1, 0, 5000)
    got = check(monkeypatch, emu_table, accs, dks, sc.Logs(1))     # only zeros are found
    assert [i for i, g in enumerate(got) if g[2]] == [0] and got[0][6] == 0
    got = check(monkeypatch, emu_table, accs, dks, sc.Logs(256))   # one probe per hit
    assert [(g[0], g[6]) for g in got if g[2]] == [(0, 0), (2, 2)]


def test_zero_ciphertexts(emu_lib, emu_table, logs5000, monkeypatch):
    accs, _ = bc.zero_cases(emu_lib)
    got = check(monkeypatch, emu_table, accs, [sc.WALLET, sc.ALICE, sc.BOB], logs5000)
    assert [(g[0], g[1], g[2], g[4], g[6]) for g in got] == [(0, 0, 1, 1, 7), (1, 1, 1, 1, 9), (2, 2, 1, 1, 0), (3, 0, 1, 0, 0), (4, 1, 1, 0, 0)]
    assert got[2][7] == got[3][7] == got[4][7] == bc.IDENTITY * 2          # Ciphertext::zero() as both: the identity encoding twice
    assert got[0][7] == b"".join(accs[0]["balance"]) and got[1][7] == b"".join(accs[1]["pending"])


def test_edge_scalars(emu_lib, emu_table, logs5000, monkeypatch):
    """1, 2, FS_MOD - 1 (bit 251: the top window), 2^251 and 0x0777..7 (a carry into every window), each owning one due account"""
    accs, cand = bc.edge_cases(emu_lib, [1, 255, 256, 4990, 17])
    got = check(monkeypatch, emu_table, accs, skc.EDGE, logs5000)
    assert [(g[0], g[1], g[2], g[6]) for g in got] == [(j, j, 1, cand[j]) for j in range(5)]


def test_lane_layout(emu_lib, emu_table, logs5000, monkeypatch):
    due, mixed, strangers, last, _ = bc.lane_layout_cases(emu_lib)
    got = check(monkeypatch, emu_table, due, skc.CYCLE, logs5000)
    assert [(g[0], g[1], g[2], g[6]) for g in got] == [(j, j % 5, 1, 101 + 7 * j + j % 9) for j in range(65)]
    got_mixed = check(monkeypatch, emu_table, mixed, skc.CYCLE, logs5000)
    assert [(g[0], g[4], g[6]) for g in got_mixed] == [(j, 1 - j % 2, 100 + 7 * j + (0 if j % 2 else 1 + j % 9)) for j in range(65)]
    got = check(monkeypatch, emu_table, strangers, skc.CYCLE, logs5000)
    assert len(strangers) == 129 and [(g[0], ) + g[1:] for g in got] == [(2 * g[0], ) + g[1:] for g in got_mixed]
    got = check(monkeypatch, emu_table, last, skc.CYCLE, logs5000)
    assert [(g[0], g[1], g[2], g[6]) for g in got] == [(5, 3, 1, 100 + 21 + 4)]


def test_one_key_owns_several_accounts(emu_lib, emu_table, logs5000, monkeypatch):
    accs, _ = bc.asset_cases(emu_lib)
    got = check(monkeypatch, emu_table, accs, [sc.WALLET], logs5000)
    assert [(g[0], g[1], g[4], g[6]) for g in got] == [(1, 0, 1, 11), (2, 0, 0, 20), (4, 0, 1, 33)]
    got = check(monkeypatch, emu_table, accs, [sc.WALLET, sc.ALICE], logs5000)
    assert [(g[0], g[1], g[6]) for g in got] == [(0, 1, 3), (1, 0, 11), (2, 0, 20), (3, 1, 3), (4, 0, 33)]


def test_refusals(emu_lib, emu_table, logs5000, monkeypatch):
    """each of the four fields refused in each of the three ways, the first in order when two are bad, neighbours untouched; a bad
    pending on an account that is not due is no refusal, and a stranger's account is not looked at"""
    import zero_chain_amd as zk
    accs, _, want = bc.refusal_cases(emu_lib)
    got = check(monkeypatch, emu_table, accs, [sc.WALLET, sc.ALICE], logs5000)
    by = {g[0]: g for g in got}
    assert sorted(by) == [i for i in range(18) if i != 16]
    assert {i: g[3] for i, g in by.items() if g[3]} == want and len(want) == 13
    assert all(by[i][2] == 0 and by[i][6] == 0 and by[i][7] == bytes(64) and by[i][4] == 1 for i in want)
    assert [(by[i][2], by[i][6]) for i in (0, 13, 15, 17)] == [(1, 42), (1, 44), (1, 61), (1, 42)] and by[15][4] == 0
    with zk.ScanKeys([sc.WALLET, sc.ALICE], lib=emu_lib) as keys:
        res = emu_table.balances(accs, keys, limit=5000)
    assert res[0] == (0, 0, dict(value=42, enc_total=by[0][7], pending_added=True, refusal=None))
    assert res[4][2] == dict(value=None, enc_total=None, pending_added=True, refusal=("balance_right", "not in the field"))
    assert res[12][2]["refusal"] == ("pending_right", "not in the prime-order subgroup") and res[8][2]["refusal"] == ("pending_left", "not on the curve")


def arguments(lib, table, monkeypatch):
    """hits_cap and the sizing call, every null combination, the limits, n_accounts == 0 - in both forms"""
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    accs, _ = bc.asset_cases(lib)
    arr = zk._api._account_array(accs)
    n, hits = len(arr), 5
    with zk.ScanKeys([sc.WALLET, sc.ALICE], lib=lib) as keys:
        fn = lib.zk_balance_keys
        for form in (HOST, DEVICE):
            monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", form)
            for limit in (0, (1 << 32) + 1):
                with pytest.raises(zk.ZkError) as e:
                    table.balances(accs, keys, limit=limit)
                assert e.value.variant == "InvalidArgument" and "limit" in str(e.value)
            assert table.balances([], keys) == [] == table.balances(b"", keys)
            out, count = (_lib.BalanceHit * 7)(), C.c_size_t(77)
            C.memset(out, 0xa5, C.sizeof(out))
            # hits_cap one too small: the count needed, nothing written - also as a sizing call without an array
            for o, cap in ((out, hits - 1), (None, 0)):
                with pytest.raises(zk.ZkError) as e:
                    lib.check(fn(table._h, keys._h, n, arr, 5000, o, cap, C.byref(count)))
                assert e.value.variant == "InvalidArgument" and "hits_cap" in str(e.value) and count.value == hits
                assert bytes(out) == b"\xa5" * C.sizeof(out)
            assert fn(table._h, keys._h, n, arr, 5000, out, hits, C.byref(count)) == 0 and count.value == hits
            assert bytes(out)[80 * hits:] == b"\xa5" * 80 * (7 - hits) and [(o.account, o.key, o.r.value) for o in out[:hits]] == [(0, 1, 3), (1, 0, 11), (2, 0, 20), (3, 1, 3), (4, 0, 33)]
            for args in ((None, keys._h, n, arr, 5000, out, 7, C.byref(count)), (table._h, None, n, arr, 5000, out, 7, C.byref(count)),
                         (table._h, keys._h, n, arr, 5000, out, 7, None), (table._h, keys._h, n, None, 5000, out, 7, C.byref(count)),
                         (table._h, keys._h, n, arr, 5000, None, 7, C.byref(count)), (None, None, 0, None, 5000, None, 0, None)):
                with pytest.raises(zk.ZkError) as e:
                    lib.check(fn(*args))
                assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
            count.value = 77
            assert fn(table._h, keys._h, 0, None, 5000, None, 0, C.byref(count)) == 0 and count.value == 0   # n_accounts == 0
            # strangers only: no hit, nothing written, no array needed
            with zk.ScanKeys(skc.STRANGERS, lib=lib) as others:
                count.value = 77
                assert fn(table._h, others._h, n, arr, 5000, None, 0, C.byref(count)) == 0 and count.value == 0


def test_invalid_arguments(emu_lib, emu_table, monkeypatch):
    arguments(emu_lib, emu_table, monkeypatch)


def mirror(lib, table, monkeypatch):
    """a list of dicts, a packed array and raw bytes; accounts_out of a block executor as the input; the one-key convenience"""
    import xt_verify_cases as xc
    import zero_chain_amd as zk
    accs, _ = bc.asset_cases(lib)
    arr = zk._api._account_array(accs)
    for form in (HOST, DEVICE):
        monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", form)
        with zk.ScanKeys([sc.WALLET, sc.ALICE], lib=lib) as keys:
            res = table.balances(accs, keys, limit=5000)
            assert [(r[0], r[1], r[2]["value"], r[2]["pending_added"], r[2]["refusal"]) for r in res] == \
                [(0, 1, 3, True, None), (1, 0, 11, True, None), (2, 0, 20, False, None), (3, 1, 3, False, None), (4, 0, 33, True, None)]
            assert table.balances(arr, keys, limit=5000) == res == table.balances(bytes(arr), keys, limit=5000) == zk.balances_keys(table, accs, keys, 5000)
            with pytest.raises(ValueError):
                table.balances(bytes(arr)[:-1], keys)
        # a block without extrinsics copies its accounts through (one account per key there): what it returns goes straight in
        edge, cand = bc.edge_cases(lib, [1, 255, 256, 4990, 17])
        pvk = zk.prepare_verifying_key(xc.small_conf_key()[1], lib=lib)
        try:
            _, accounts_out, _ = zk.execute_confidential_block(pvk, [], edge, [], zk.g_epoch(3, lib=lib))
        finally:
            pvk.close()
        with zk.ScanKeys(skc.EDGE, lib=lib) as keys:
            out = table.balances(accounts_out, keys, limit=5000)
            assert out == table.balances(edge, keys, limit=5000) and [(r[0], r[1], r[2]["value"]) for r in out] == [(j, j, cand[j]) for j in range(5)]
        one = zk.balance(table, accs[4], sc.WALLET, 5000)
        assert one == res[4][2] and one["enc_total"] == zk.balance_query(sc.WALLET, accs[4]["balance"], accs[4]["pending"], table=table, limit=5000)[1]
        assert zk.balance(table, accs[2], sc.WALLET, 10)["value"] is None
        with pytest.raises(ValueError):
            zk.balance(table, accs[0], sc.WALLET, 5000)


def test_the_mirror(emu_lib, emu_table, monkeypatch):
    mirror(emu_lib, emu_table, monkeypatch)


def test_balance_combine_kernel_keeps_its_table_in_lds():
    """the code object's metadata for k_balance_combine: one such kernel, no scratch memory, LDS within k_rj_check's budget"""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources(_lib.LIB_PATH).items() if "k_balance_combine" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and r["lds"] <= 36864, r


# ---------------------------------------------------------------------------------------------- GPU
BIG = [0, 1, 999999, 10 ** 6, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 32) - 1]


@pytest.fixture(scope="module")
def table(gpu_lib):
    import zero_chain_amd as zk
    t = zk.ElGamalTable(lib=gpu_lib)
    yield t
    t.close()


@pytest.mark.gpu
def test_gpu_values_zeros_edge_scalars_and_refusals(gpu_lib, table, monkeypatch):
    accs, cand = bc.value_cases(gpu_lib, BIG, 10 ** 6)
    zeros, cand1 = bc.zero_cases(gpu_lib)
    edge, cand2 = bc.edge_cases(gpu_lib, BIG[3:])
    bad, cand3, want = bc.refusal_cases(gpu_lib)
    assets, cand4 = bc.asset_cases(gpu_lib)
    for limit in (10 ** 6, 1 << 32):
        logs = sc.Logs(limit, cand + cand1 + cand2 + cand3 + cand4)
        got = check(monkeypatch, table, accs, [sc.ALICE, sc.WALLET], logs)
        # 999999 + 1 reaches 10^6 only with the pending; with the bit clear 999999 is found at either limit
        assert got[-2][2:7] == ((0, 0, 1, 0, 0) if limit == 10 ** 6 else (1, 0, 1, 0, 10 ** 6)) and got[-1][2:7] == (1, 0, 0, 0, 999999)
        assert all(g[2] == 1 for g in got) or limit == 10 ** 6
        got = check(monkeypatch, table, zeros, [sc.WALLET, sc.ALICE, sc.BOB], logs)
        assert [g[6] for g in got] == [7, 9, 0, 0, 0] and got[2][7] == bc.IDENTITY * 2
        got = check(monkeypatch, table, edge, skc.EDGE, logs)
        assert [g[6] for g in got if g[2]] == [c for c in cand2 if c < limit]
        got = check(monkeypatch, table, bad, [sc.WALLET, sc.ALICE], logs)
        assert {g[0]: g[3] for g in got if g[3]} == want
        assert len(check(monkeypatch, table, assets, [sc.WALLET], logs)) == 3


@pytest.mark.gpu
def test_gpu_lane_layout(gpu_lib, table, monkeypatch):
    due, mixed, strangers, last, _ = bc.lane_layout_cases(gpu_lib)
    logs = sc.Logs(5000)
    assert len(check(monkeypatch, table, due, skc.CYCLE, logs)) == 65
    assert len(check(monkeypatch, table, mixed, skc.CYCLE, logs)) == 65
    assert len(check(monkeypatch, table, strangers, skc.CYCLE, logs)) == 65
    assert [g[0] for g in check(monkeypatch, table, last, skc.CYCLE, logs)] == [5]


@pytest.mark.gpu
def test_gpu_random_accounts_of_forty_keys(gpu_lib, table, monkeypatch):
    """300 accounts over 40 keys and 20 strangers, one in three not due, one in four with an empty pending: the expectation is the
    plaintexts the accounts were built from (the oracle holds the small cases above) and the two-call route's bytes"""
    import zero_chain_amd as zk
    rng = random.Random(43)
    dks = sc.fs(106, 60)
    amount = lambda: rng.randrange(10 ** 6) if rng.randrange(3) else rng.randrange(10 ** 6, 1 << 31)
    specs = [(rng.choice(dks), amount(), None if rng.randrange(4) == 0 else amount(), 0 if rng.randrange(3) == 0 else bc.DUE) for _ in range(300)]
    accs = bc.accounts(gpu_lib, specs, 48)
    number = {dk: k for k, dk in enumerate(dks[:40])}
    with zk.ScanKeys(dks[:40], lib=gpu_lib) as keys:
        for limit in (10 ** 6, 1 << 32):
            got = both_forms(monkeypatch, table, accs, keys, limit)
            want = [bc.plain_hit(i, number[s[0]], s[1], s[2], s[3], limit, g[16:]) for (i, s), g in
                    zip(((i, s) for i, s in enumerate(specs) if s[0] in number), got)]
            assert got == want and 150 < len(got) < 250
            two_calls(table, accs, dks, got, limit)
    assert sum(1 for s in specs if s[2] is None) > 50 and sum(1 for s in specs if not s[3]) > 70


@pytest.mark.gpu
def test_gpu_arguments_and_the_mirror(gpu_lib, table, monkeypatch):
    arguments(gpu_lib, table, monkeypatch)
    mirror(gpu_lib, table, monkeypatch)


@pytest.mark.gpu
def test_gpu_balance_memory_is_returned_and_wiped(gpu_lib, monkeypatch):
    import zero_chain_amd as zk
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    accs, _ = bc.asset_cases(gpu_lib)
    before = zk.memory_stats(lib=gpu_lib)
    with zk.ScanKeys([sc.WALLET, sc.ALICE], lib=gpu_lib) as keys:
        with zk.ElGamalTable(lib=gpu_lib) as t:
            built = zk.memory_stats(lib=gpu_lib)["device_held"]
            res = t.balances(accs, keys, limit=1 << 32)
            assert [(r[0], r[1], r[2]["value"]) for r in res] == [(0, 1, 3), (1, 0, 11), (2, 0, 20), (3, 1, 3), (4, 0, 33)]
            assert zk.memory_stats(lib=gpu_lib)["device_held"] > built   # the stage's buffers stay with the table
    after = zk.memory_stats(lib=gpu_lib)
    assert after["device_held"] == before["device_held"]
    assert after["device_released"] == after["device_wiped"] > before["device_released"]
