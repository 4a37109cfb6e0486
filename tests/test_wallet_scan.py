"""A block read with one decryption key (zk_confidential_scan / zk_anonymous_scan, csrc/elgamal_scan.h): which extrinsics touch
the wallet's key and by how much - Ciphertext::decrypt (core/proofs/src/no_std_aliases/elgamal.rs:85-108) per value, the signs
of MultiCiphertexts::<Anonymous>::encrypt (core/proofs/src/crypto_components.rs:168-220).  Every case runs with the host form
of the point work forced (ZKAMD_SCAN_HOST_MAX large) and with the two kernels forced (0): the two result arrays must be equal
byte for byte, and equal to the expectation tests/scan_cases.py computes with oracle/jubjub.py.
CPU: the x86 emulation build of the kernel sources with 8 baby-step bits and limit 5000 (k_dlog_probe at limit 256, k_dlog_search
above).  GPU: the product library with the default table, limits 10^6 and 2^32."""
import ctypes as C
import os
import random

import pytest

import scan_cases as sc
from oracle import jubjub as jj

HOST, DEVICE = str(1 << 40), "0"


def scan_raw(table, kind, xts, dk, limit):
    """the result array of the C entry as bytes, through the mirror's own marshalling"""
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    if kind == "confidential":
        res = table._scan(table._lib.zk_confidential_scan, _lib.ConfidentialXt, zk._api._fill_confidential_xt, _lib.ConfidentialScanResult, xts, dk, limit)
    else:
        res = table._scan(table._lib.zk_anonymous_scan, _lib.AnonymousXt, zk._api._fill_anonymous_xt, _lib.AnonymousScanResult, xts, dk, limit)
    return [bytes(r) for r in res]


def both_forms(monkeypatch, table, kind, xts, dk, limit):
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", HOST)
    host = scan_raw(table, kind, xts, dk, limit)
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    device = scan_raw(table, kind, xts, dk, limit)
    assert host == device, [k for k in range(len(host)) if host[k] != device[k]]
    return host


def check(monkeypatch, table, kind, xts, dk, logs):
    want = [(sc.expected_confidential if kind == "confidential" else sc.expected_anonymous)(x, dk, logs) for x in xts]
    got = both_forms(monkeypatch, table, kind, xts, dk, logs.limit)
    assert got == want, [(k, got[k].hex(), want[k].hex()) for k in range(len(want)) if got[k] != want[k]]
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
def test_confidential_roles(emu_lib, emu_table, logs5000, monkeypatch):
    import zero_chain_amd as zk
    xts, _ = sc.confidential_role_cases(emu_lib, [0, 1, 255, 256, 257, 4999, 5000], 70000, 5000)
    got = check(monkeypatch, emu_table, "confidential", xts, sc.WALLET, logs5000)
    # spelled out for a few: 4999 as sender / recipient / to oneself, 5000 to oneself (the fee still found), neither, the fees,
    # and a ciphertext under a stranger's key
    res = emu_table.scan_confidential(xts, sc.WALLET, limit=5000)
    none = dict(refusal=None, amount_sent=None, fee=None, amount_received=None)
    assert res[15] == dict(none, role=zk.SCAN_SENDER, amount_sent=4999, fee=3)
    assert res[16] == dict(none, role=zk.SCAN_RECIPIENT, amount_received=4999)
    assert res[17] == dict(none, role=3, amount_sent=4999, fee=1, amount_received=4999)
    assert res[20] == dict(none, role=3, fee=1)
    assert res[21] == dict(none, role=0)
    assert res[22] == dict(none, role=zk.SCAN_SENDER, amount_sent=7, fee=0)
    assert res[23] == dict(none, role=zk.SCAN_SENDER, amount_sent=7)
    assert res[24] == dict(none, role=zk.SCAN_RECIPIENT)
    assert got[21] == bytes(16)
    # the same bytes from the packed array and from raw bytes; limit 256 is one probe per value
    from zero_chain_amd import _lib
    arr = zk._api._xt_array(xts, _lib.ConfidentialXt, zk._api._fill_confidential_xt)
    assert emu_table.scan_confidential(arr, sc.WALLET, limit=5000) == res == emu_table.scan_confidential(bytes(arr), sc.WALLET, limit=5000)
    check(monkeypatch, emu_table, "confidential", xts[:12], sc.WALLET, sc.Logs(256))
    # another wallet reads the same block
    check(monkeypatch, emu_table, "confidential", xts, sc.ALICE, logs5000)


def test_anonymous_members_signs_and_sums(emu_lib, emu_table, logs5000, monkeypatch):
    xts, _ = sc.anonymous_cases(emu_lib, [1, 255, 256, 257, 4999], 5000)
    check(monkeypatch, emu_table, "anonymous", xts, sc.WALLET, logs5000)
    res = emu_table.scan_anonymous(xts, sc.WALLET, limit=5000)
    assert res[0] == dict(members=[], refusal=None, delta=None)
    assert res[1] == dict(members=[5], refusal=None, delta=0)
    assert [r["delta"] for r in res[2:12]] == [1, -1, 255, -255, 256, -256, 257, -257, 4999, -4999]
    assert [r["delta"] for r in res[12:14]] == [None, None] and res[12]["members"] == [2]
    assert res[14] == dict(members=[0], refusal=None, delta=1) and res[15] == dict(members=[11], refusal=None, delta=-4999)
    assert res[16] == dict(members=[4, 9], refusal=None, delta=255)
    assert res[17] == dict(members=[1, 10], refusal=None, delta=293)
    assert res[18] == dict(members=[0, 11], refusal=None, delta=None) and res[19] == dict(members=[3, 6], refusal=None, delta=None)
    # limit 1: only zeros are found
    got = check(monkeypatch, emu_table, "anonymous", xts, sc.WALLET, sc.Logs(1))
    found = [k for k, g in enumerate(got) if g[2]]
    assert found == [1], found
    check(monkeypatch, emu_table, "anonymous", xts, sc.WALLET, sc.Logs(256))
    check(monkeypatch, emu_table, "anonymous", xts, sc.BOB, logs5000)   # absent everywhere


def test_refusals_are_results(emu_lib, emu_table, logs5000, monkeypatch):
    import zero_chain_amd as zk
    cx, ax, _ = sc.refusal_cases(emu_lib)
    got = check(monkeypatch, emu_table, "confidential", cx, sc.WALLET, logs5000)
    assert [g[2] for g in got] == [0, 0, 0, 4 | 3 << 6, 5 | 1 << 6, 6 | 2 << 6, 3 | 1 << 6, 0, 0, 0, 0, 0, 0]
    assert [g[0] for g in got[7:10]] == [sc.RECIPIENT, 0, 0] and got[7][1] == sc.FOUND_RECEIVED
    res = emu_table.scan_confidential(cx, sc.WALLET, limit=5000)
    assert res[3] == dict(role=2, refusal=("left_amount_recipient", "not in the prime-order subgroup"), amount_sent=None, fee=None, amount_received=None)
    assert res[4]["refusal"] == ("right_randomness", "not in the field") and res[5]["refusal"] == ("left_fee", "not on the curve")
    assert res[10:] == res[:3] and res[0]["amount_received"] == 40 and res[2]["fee"] == 3   # the neighbours are unaffected
    got = check(monkeypatch, emu_table, "anonymous", ax, sc.WALLET, logs5000)
    assert [g[3] for g in got] == [0, 19 | 3 << 6, 20 | 1 << 6, 49 | 2 << 6, 0, 0, 0]
    res = emu_table.scan_anonymous(ax, sc.WALLET, limit=5000)
    assert res[1] == dict(members=[6], refusal=("left_ciphertexts[6]", "not in the prime-order subgroup"), delta=None)
    assert res[3]["refusal"] == ("right_ciphertext", "not on the curve") and res[0]["delta"] == res[6]["delta"] == 17
    assert res[4] == res[5] == dict(members=[], refusal=None, delta=None)


def test_invalid_arguments(emu_lib, emu_table, monkeypatch):
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    cx = sc.confidential_xts(emu_lib, [(sc.ALICE, sc.WALLET, 5, 1)])
    ax = sc.anonymous_xts(emu_lib, [sc.ring(emu_lib, zk.jubjub_base_mul([sc.WALLET], lib=emu_lib)[0], {4: 5})])
    for form in (HOST, DEVICE):
        monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", form)
        for scan, xts in ((emu_table.scan_confidential, cx), (emu_table.scan_anonymous, ax)):
            with pytest.raises(zk.ZkError) as e:
                scan(xts, jj.FS_MOD, limit=5000)
            assert e.value.variant == "InvalidArgument" and "dec_key is not a canonical Fs scalar" in str(e.value)
            for limit in (0, (1 << 32) + 1):
                with pytest.raises(zk.ZkError) as e:
                    scan(xts, sc.WALLET, limit=limit)
                assert e.value.variant == "InvalidArgument" and "limit" in str(e.value)
            assert scan([], sc.WALLET) == [] and scan(b"", sc.WALLET) == []
    # the raw entries: NULLs with n > 0; n == 0 touches nothing (no pointer is read or written)
    key = C.create_string_buffer(sc.WALLET.to_bytes(32, "little"), 32)
    carr = zk._api._xt_array(cx, _lib.ConfidentialXt, zk._api._fill_confidential_xt)
    aarr = zk._api._xt_array(ax, _lib.AnonymousXt, zk._api._fill_anonymous_xt)
    cout, aout = (_lib.ConfidentialScanResult * 1)(), (_lib.AnonymousScanResult * 1)()
    for fn, arr, out in ((emu_lib.zk_confidential_scan, carr, cout), (emu_lib.zk_anonymous_scan, aarr, aout)):
        assert fn(emu_table._h, 1, arr, key, 5000, out) == 0
        for args in ((None, 1, arr, key, 5000, out), (emu_table._h, 1, None, key, 5000, out), (emu_table._h, 1, arr, None, 5000, out),
                     (emu_table._h, 1, arr, key, 5000, None), (None, 0, None, None, 5000, None)):
            with pytest.raises(zk.ZkError) as e:
                emu_lib.check(fn(*args))
            assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
        assert fn(emu_table._h, 0, None, None, 5000, None) == 0
    assert (cout[0].role, cout[0].found, cout[0].amount_received) == (2, 4, 5) and (aout[0].members, aout[0].found, aout[0].delta) == (16, 1, 5)


def test_lane_layout_gather_and_scatter(emu_lib, emu_table, logs5000, monkeypatch):
    own, mixed, last, _ = sc.lane_layout_cases(emu_lib)
    got = check(monkeypatch, emu_table, "confidential", own, sc.WALLET, logs5000)
    assert all(g[0] == 3 and g[1] == 7 for g in got)
    got_mixed = check(monkeypatch, emu_table, "confidential", mixed, sc.WALLET, logs5000)
    assert got_mixed[1::2] == [bytes(16)] * 22
    assert [g[:2] + g[4:] for g in got_mixed[0::2]] == [g[:2] + g[4:] for g in got]
    got = check(monkeypatch, emu_table, "confidential", last, sc.WALLET, logs5000)
    assert got[:5] == [bytes(16)] * 5 and got[5][:2] == bytes([sc.RECIPIENT, sc.FOUND_RECEIVED])


# ---------------------------------------------------------------------------------------------- GPU
BIG = [0, 1, 999999, 10 ** 6, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 32) - 1]


@pytest.fixture(scope="module")
def table(gpu_lib):
    import zero_chain_amd as zk
    t = zk.ElGamalTable(lib=gpu_lib)
    yield t
    t.close()


@pytest.mark.gpu
def test_gpu_confidential_roles_and_refusals(gpu_lib, table, monkeypatch):
    xts, cand = sc.confidential_role_cases(gpu_lib, BIG, (1 << 31) + 5, 10 ** 6)
    cx, _, cand2 = sc.refusal_cases(gpu_lib)
    for limit in (10 ** 6, 1 << 32):
        logs = sc.Logs(limit, cand + cand2)
        got = check(monkeypatch, table, "confidential", xts, sc.WALLET, logs)
        # to oneself with 2^32 - 1: all three values at 2^32, only the fee at 10^6
        assert got[23][:2] == bytes([3, 7 if limit > 10 ** 6 else sc.FOUND_FEE])
        got = check(monkeypatch, table, "confidential", cx, sc.WALLET, logs)
        assert [g[2] for g in got] == [0, 0, 0, 4 | 3 << 6, 5 | 1 << 6, 6 | 2 << 6, 3 | 1 << 6, 0, 0, 0, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_anonymous_signs_and_refusals(gpu_lib, table, monkeypatch):
    xts, cand = sc.anonymous_cases(gpu_lib, BIG[1:], (1 << 32) - 2)
    _, ax, cand2 = sc.refusal_cases(gpu_lib)
    for limit in (10 ** 6, 1 << 32):
        logs = sc.Logs(limit, cand + cand2)
        check(monkeypatch, table, "anonymous", xts, sc.WALLET, logs)
        got = check(monkeypatch, table, "anonymous", ax, sc.WALLET, logs)
        assert [g[3] for g in got] == [0, 19 | 3 << 6, 20 | 1 << 6, 49 | 2 << 6, 0, 0, 0]
    res = table.scan_anonymous(xts, sc.WALLET, limit=1 << 32)
    assert [r["delta"] for r in res[2:6]] == [1, -1, 999999, -999999] and res[15]["delta"] == -((1 << 32) - 1)
    with pytest.raises(__import__("zero_chain_amd").ZkError) as e:
        table.scan_anonymous(xts, jj.FS_MOD)
    assert "dec_key" in str(e.value)


@pytest.mark.gpu
def test_gpu_random_block_spans_several_waves_of_both_kinds(gpu_lib, table, monkeypatch):
    """300 confidential and 300 anonymous extrinsics, about a third of them strangers': the expectation here is the plaintext each
    was built from (the oracle holds the small cases above), and ElGamalTable.decrypt on the recipient's pairs"""
    import struct
    import zero_chain_amd as zk
    rng = random.Random(21)
    (w,) = zk.jubjub_base_mul([sc.WALLET], lib=gpu_lib)
    amount = lambda: rng.randrange(10 ** 6) if rng.randrange(3) else rng.randrange(10 ** 6, 1 << 32)
    roles = [rng.choice((0, 1, 2, 3, 1, 2)) for _ in range(300)]
    specs = [(sc.WALLET if r & 1 else sc.ALICE, sc.WALLET if r & 2 else sc.BOB, amount(), rng.randrange(1000)) for r in roles]
    cx = sc.confidential_xts(gpu_lib, specs, seed=22)
    aspecs, placed = [], []
    for _ in range(300):
        p = {} if not rng.randrange(3) else {rng.randrange(12): rng.choice((0, 1, -1)) * amount()}
        placed.append(p)
        aspecs.append(sc.ring(gpu_lib, w, p))
    ax = sc.anonymous_xts(gpu_lib, aspecs, seed=23)
    for limit, n in ((10 ** 6, 300), (1 << 32, 64)):
        val = lambda v: (1, v) if v < limit else (0, 0)
        want = []
        for r, (_, _, a, f) in zip(roles[:n], specs[:n]):
            s, fee, rec = (val(a) if r & 1 else (0, 0)), (val(f) if r & 1 else (0, 0)), (val(a) if r & 2 else (0, 0))
            want.append(struct.pack("<BBBBIII", r, s[0] | fee[0] << 1 | rec[0] << 2, 0, 0, s[1], fee[1], rec[1]))
        got = both_forms(monkeypatch, table, "confidential", cx[:n], sc.WALLET, limit)
        assert got == want
        mine = [k for k in range(n) if roles[k] & 2]
        dec = table.decrypt([cx[k]["left_amount_recipient"] for k in mine], [cx[k]["right_randomness"] for k in mine], sc.WALLET, limit=limit)
        assert dec == [struct.unpack("<I", got[k][12:])[0] if got[k][1] & 4 else None for k in mine]
        want = []
        for p in placed[:n]:
            ((k, v),) = p.items() or ((0, None),)
            ok = v is not None and abs(v) < limit
            want.append(bytes(16) if v is None else struct.pack("<HBBIq", 1 << k, ok, 0, 0, v if ok else 0))
        assert both_forms(monkeypatch, table, "anonymous", ax[:n], sc.WALLET, limit) == want


@pytest.mark.gpu
def test_gpu_scan_reads_what_gen_proof_wrote(gpu_lib, table, monkeypatch):
    """zk_transfer_gen_proof_batch / zk_anonymous_gen_proof_batch under the toxic-waste key of tests/helpers.py, then the scan of the
    extrinsic: the sender finds amount and fee (-amount in the ring), the recipient the amount, a decoy 0"""
    import helpers
    import zero_chain_amd as zk
    import test_gen_proof as tg
    recipient, decoy = sc.fs(31, 2)
    rkey, dkey = zk.jubjub_base_mul([recipient, decoy], lib=gpu_lib)
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    for circuit in ("transfer", "anonymous"):
        mats = (zk.ConstraintMatrices.transfer_circuit if circuit == "transfer" else zk.ConstraintMatrices.anonymous_circuit)(lib=gpu_lib)
        params = pvk = None
        try:
            params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=gpu_lib)
            pvk = zk.prepare_verifying_key(params)
            if circuit == "transfer":
                rq = dict(tg.reference_request(3)[0], enc_key_recipient=rkey)
                st, _ = zk.transfer_derive(zk.transfer_requests([rq]), lib=gpu_lib)
                sender = int.from_bytes(bytes(st[0].dec_key_sender), "little")
                raw = zk.gen_proofs(params, mats, pvk, zk.transfer_requests([rq]), [(5, 6)], raw=True)
                none = dict(refusal=None, amount_sent=None, fee=None, amount_received=None)
                assert table.scan_confidential(raw, sender) == [dict(none, role=zk.SCAN_SENDER, amount_sent=rq["amount"], fee=rq["fee"])]
                assert table.scan_confidential(raw, recipient) == [dict(none, role=zk.SCAN_RECIPIENT, amount_received=rq["amount"])]
                assert table.scan_confidential(raw, decoy) == [dict(none, role=0)]
            else:
                rq = tg.anonymous_request(2)[0]
                rq = dict(rq, enc_key_recipient=rkey, enc_keys_decoy=[dkey] + rq["enc_keys_decoy"][1:])
                st, _ = zk.anonymous_derive(zk.anonymous_requests([rq]), lib=gpu_lib)
                sender = int.from_bytes(bytes(st[0].dec_key), "little")
                xts = zk.anonymous_gen_proofs(params, mats, pvk, zk.anonymous_requests([rq]), [(7, 8)])
                at = min(k for k in range(12) if k not in (rq["s_index"], rq["t_index"]))
                assert table.scan_anonymous(xts, sender) == [dict(members=[rq["s_index"]], refusal=None, delta=-rq["amount"])]
                assert table.scan_anonymous(xts, recipient) == [dict(members=[rq["t_index"]], refusal=None, delta=rq["amount"])]
                assert table.scan_anonymous(xts, decoy) == [dict(members=[at], refusal=None, delta=0)]
        finally:
            for h in (pvk, params, mats):
                if h is not None:
                    h.close()


@pytest.mark.gpu
def test_gpu_scan_memory_is_returned_and_wiped(gpu_lib, monkeypatch):
    import zero_chain_amd as zk
    monkeypatch.setenv("ZKAMD_SCAN_HOST_MAX", DEVICE)
    xts = sc.confidential_xts(gpu_lib, [(sc.WALLET, sc.WALLET, 5, 1), (sc.ALICE, sc.WALLET, 123456789, 2)])
    before = zk.memory_stats(lib=gpu_lib)
    with zk.ElGamalTable(lib=gpu_lib) as t:
        built = zk.memory_stats(lib=gpu_lib)["device_held"]
        res = t.scan_confidential(xts, sc.WALLET, limit=1 << 32)
        assert [r["amount_received"] for r in res] == [5, 123456789]
        assert zk.memory_stats(lib=gpu_lib)["device_held"] > built   # the stage's buffers stay with the table
    after = zk.memory_stats(lib=gpu_lib)
    assert after["device_held"] == before["device_held"]
    assert after["device_released"] == after["device_wiped"] > before["device_released"]


def test_scan_points_kernel_keeps_its_tables_in_lds():
    """the code object's metadata for k_scan_points: 16 slots x 32 bytes x 64 lanes of LDS and no scratch memory, as k_into_xy
    (tests/test_xt_verify.py, through the same helper)"""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources(_lib.LIB_PATH).items() if "k_scan_points" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and r["lds"] == 32768, r
