"""The request -> statement derivation of the anonymous transfer as a stage with a device form (zk_anonymous_derive_dev and the
front end of zk_anonymous_gen_proof_batch; csrc/anon_derive.h) against the Python model of tests/anon_derive_cases.py.

Every case runs on the x86 emulation build and, marked gpu, on the product library, each time with the host form forced
(ZKAMD_ANON_DERIVE_HOST_MAX large) and with the kernels forced (0): the two outputs - statements, rsk, the 104 public inputs -
must be equal byte for byte, and a refusal must carry the same variant and message.  Model-checked requests stay at or below 6
per test (13 point multiplications each in Python, computed once per distinct request); larger counts compare the two forms
alone.  No test runs more than about 520 lanes of a kernel: 13 requests are 65 fixed-base, 156 variable-base, 208 combine and at
most 468 decode lanes."""
import ctypes as C
import os

import pytest

import anon_derive_cases as ad
import scan_cases as sc
from oracle import jubjub as jj

HOST, DEVICE = str(1 << 40), "0"
VAR = "ZKAMD_ANON_DERIVE_HOST_MAX"
STAGES = ("anon_derive_points", "anon_derive_combine")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "gpu_lib")


def raw(result):
    st, rsks, inputs = result
    return bytes(st), rsks, inputs


def both_forms(monkeypatch, lib, rqs):
    """(statements, rsks, inputs) of the batch, the same from both forms"""
    import zero_chain_amd as zk
    arr = zk.anonymous_requests(rqs)
    monkeypatch.setenv(VAR, HOST)
    host = zk.anonymous_derive_dev(arr, want_inputs=True, lib=lib)
    monkeypatch.setenv(VAR, DEVICE)
    device = zk.anonymous_derive_dev(arr, want_inputs=True, lib=lib)
    assert raw(host) == raw(device)
    # ... and the host-only entry writes the same statements
    plain = zk.anonymous_derive(arr, lib=lib)
    assert bytes(plain[0]) == bytes(device[0]) and plain[1] == device[1]
    return device


def check(monkeypatch, lib, rqs):
    """both forms, and the model for every request"""
    st, rsks, inputs = both_forms(monkeypatch, lib, rqs)
    for i, rq in enumerate(rqs):
        want_st, want_rsk, want_inputs, _ = ad.expected(rq)
        assert ad.statement_dict(st[i]) == want_st, i
        assert rsks[i] == want_rsk and inputs[i] == want_inputs, i
    return st, rsks, inputs


def refused(monkeypatch, lib, rqs, text):
    """both forms refuse the batch with InvalidArgument and the same message, which holds `text`"""
    import zero_chain_amd as zk
    arr = zk.anonymous_requests(rqs)
    msgs = []
    for form in (HOST, DEVICE):
        monkeypatch.setenv(VAR, form)
        with pytest.raises(zk.ZkError) as e:
            zk.anonymous_derive_dev(arr, want_inputs=True, lib=lib)
        assert e.value.variant == "InvalidArgument", str(e.value)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and text in msgs[0], (text, msgs)
    with pytest.raises(zk.ZkError) as e:
        zk.anonymous_derive(arr, lib=lib)
    assert str(e.value) == msgs[0]


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [1, 2, 6])
def test_sizes_against_the_model(lib, monkeypatch, n):
    """one request; two with nothing in common (72 decode lanes: a second wave); six (72 variable-base lanes)"""
    rqs = [ad.request(k) for k in range(n)]
    if n == 2:
        assert len({e for rq in rqs for e in [rq["enc_key_recipient"], rq["g_epoch"]] + rq["enc_keys_decoy"] + rq["enc_balances_left"] + rq["enc_balances_right"]}) == 72
    check(monkeypatch, lib, rqs)


def test_thirteen_requests_with_shared_encodings(lib, monkeypatch):
    """65 fixed-base and 208 combine lanes; one g_epoch for the batch, decoys shared between neighbours (the windows of the pool
    overlap), two requests byte-identical.  The model holds the first two."""
    g_epoch = ad.pool()[95]
    rqs = [ad.request(k, first=7 * k, g_epoch=g_epoch) for k in range(12)]
    rqs.insert(5, dict(rqs[3]))
    assert len(rqs) == 13 and rqs[5] == rqs[3]
    st, rsks, inputs = both_forms(monkeypatch, lib, rqs)
    assert bytes(st[5]) == bytes(st[3]) and rsks[5] == rsks[3] and inputs[5] == inputs[3]
    for i in (0, 1):
        want_st, want_rsk, want_inputs, _ = ad.expected(rqs[i])
        assert (ad.statement_dict(st[i]), rsks[i], inputs[i]) == (want_st, want_rsk, want_inputs)


def test_several_slices(emu_lib, monkeypatch):
    """the slice loop, with the emulation build's hook: five requests in slices of two, a refusal in the last slice.  It covers the
    pool indices: a slice's variable lanes read dk for g_epoch and r for the rest through the slice's pool, the second request of a
    slice at its own five scalars; beside the model, the nonce and a decoy's left of every request are recomputed here."""
    monkeypatch.setenv("ZKAMD_DEBUG_ANON_SLICE", "2")
    rqs = [ad.request(k) for k in range(5)]
    st, _, inputs = check(monkeypatch, emu_lib, rqs)
    for i, rq in enumerate(rqs):   # the nonce [dk] g_epoch and a decoy's left [r] key, from the request's own scalars
        d, m = ad.statement_dict(st[i]), next(m for m in range(12) if m not in (rq["s_index"], rq["t_index"]))
        assert inputs[i][2 * 51:2 * 52] == list(jj.mul(jj.read_point(rq["g_epoch"]), d["dec_key"]))
        assert d["left_ciphertexts"][m] == jj.write_point(jj.mul(jj.read_point(d["enc_keys"][m]), rq["randomness"]))
    rqs[4] = dict(rqs[4], g_epoch=sc.NOT_A_POINT)
    refused(monkeypatch, emu_lib, rqs, "request 4: g_epoch is not a Jubjub point")


@pytest.mark.parametrize("s_index,t_index", [(0, 11), (11, 0), (5, 6), (6, 5)])
def test_set_positions(lib, monkeypatch, s_index, t_index):
    st, _, _ = check(monkeypatch, lib, [ad.request(3, s_index=s_index, t_index=t_index)])
    rq = ad.request(3, s_index=s_index, t_index=t_index)
    keys = [bytes(e) for e in st[0].enc_keys]
    assert keys[t_index] == rq["enc_key_recipient"] and [k for i, k in enumerate(keys) if i not in (s_index, t_index)] == rq["enc_keys_decoy"]


# ---------------------------------------------------------------------------------------------- edge values
def test_edge_amounts_and_randomness(lib, monkeypatch):
    top = (1 << 32) - 1
    rqs = [ad.request(0, amount=0, balance=0),
           ad.request(1, amount=top, balance=top),
           ad.request(2, amount=0, randomness=0),                       # every ciphertext the identity
           ad.request(3, amount=77, randomness=0),                      # r dk < amount: u wraps; left = -[77]G, +[77]G, O ...
           ad.request(4, randomness=jj.FS_MOD - 1),
           ad.request(5, amount=top, balance=top, randomness=1)]        # u = dk - amount
    st, _, inputs = check(monkeypatch, lib, rqs)
    left = [bytes(e) for e in st[2].left_ciphertexts]
    assert left == [ad.IDENTITY] * 12 and inputs[2][2 * 48:2 * 49] == [0, 1]
    left, rq = [bytes(e) for e in st[3].left_ciphertexts], rqs[3]
    g77 = jj.mul(ad.G, 77)
    assert left[rq["s_index"]] == jj.write_point(sc.neg(g77)) and left[rq["t_index"]] == jj.write_point(g77)
    assert sorted(set(left) - {left[rq["s_index"]], left[rq["t_index"]]}) == [ad.IDENTITY]


def test_edge_alpha_and_keys(lib, monkeypatch):
    base = ad.request(1)
    own = ad.expected(base)[3]["enc_keys"][base["s_index"]]           # the sender's own [dk]G
    decoys = base["enc_keys_decoy"]
    whole_member = lambda rq, i: dict(rq, enc_balances_left=rq["enc_balances_left"][:i] + [ad.IDENTITY] + rq["enc_balances_left"][i + 1:],
                                      enc_balances_right=rq["enc_balances_right"][:i] + [ad.IDENTITY] + rq["enc_balances_right"][i + 1:])
    rqs = [dict(base, alpha=0),
           dict(base, alpha=jj.FS_MOD - base["spending_key"]),          # rvk the identity, rsk zero
           dict(base, enc_keys_decoy=[base["enc_key_recipient"]] + decoys[1:]),
           dict(base, enc_key_recipient=own),
           dict(base, enc_keys_decoy=decoys[:4] + [ad.IDENTITY] + decoys[5:]),
           whole_member(whole_member(base, 0), 7)]
    st, rsks, inputs = check(monkeypatch, lib, rqs)
    assert rsks[1] == bytes(32) and inputs[1][2 * 49:2 * 50] == [0, 1]
    assert bytes(st[3].enc_keys[base["s_index"]]) == bytes(st[3].enc_keys[base["t_index"]]) == own
    assert [bytes(e) for e in st[4].left_ciphertexts].count(ad.IDENTITY) == 1


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", [b[0] for b in ad.BAD_ENCODINGS])
def test_every_field_kind_is_refused(lib, monkeypatch, what):
    _, enc, text = next(b for b in ad.BAD_ENCODINGS if b[0] == what)
    good = ad.request(1)
    for name, put in ad.field_kinds():
        refused(monkeypatch, lib, [put(good, enc)], "request 0: %s %s" % (name, text))


def test_the_first_refusal_in_order_is_the_one_reported(lib, monkeypatch):
    a, b = ad.request(1), ad.request(2, first=36)                                  # (b shares a's points, g_epoch among them)
    kinds = dict(ad.field_kinds())
    tors, off = sc.torsion(), sc.off_curve()
    # two bad fields in one request: the earlier in field order, whatever is wrong with the later
    two = kinds["enc_balances_left[0]"](kinds["enc_keys_decoy[9]"](a, tors), off)
    refused(monkeypatch, lib, [two], "request 0: enc_keys_decoy[9] is not in the prime-order subgroup")
    two = kinds["enc_balances_right[11]"](kinds["g_epoch"](a, off), tors)
    refused(monkeypatch, lib, [two], "request 0: g_epoch is not a Jubjub point")
    # the same bad encoding in two fields (one decode lane): the earlier field is named
    two = kinds["enc_balances_right[4]"](kinds["enc_key_recipient"](a, tors), tors)
    refused(monkeypatch, lib, [two], "request 0: enc_key_recipient is not in the prime-order subgroup")
    # two bad requests: the lower index
    refused(monkeypatch, lib, [b, kinds["g_epoch"](a, off), kinds["enc_key_recipient"](b, tors)], "request 1: g_epoch is not a Jubjub point")
    # a bad request beside a good one that shares its g_epoch (and every other point)
    assert a["g_epoch"] == b["g_epoch"]
    refused(monkeypatch, lib, [a, kinds["enc_balances_left[0]"](b, ad.SMALL_ORDER)], "request 1: enc_balances_left[0] is not in the prime-order subgroup")
    refused(monkeypatch, lib, [kinds["enc_balances_left[0]"](b, ad.SMALL_ORDER), a], "request 0: enc_balances_left[0]")


def test_scalars_and_indices(lib, monkeypatch):
    a, b = ad.request(1), ad.request(2)
    kinds = dict(ad.field_kinds())
    for name in ("spending_key", "alpha", "randomness"):
        for value in (jj.FS_MOD, (1 << 256) - 1):
            refused(monkeypatch, lib, [b, dict(a, **{name: value})], "request 1: %s is not a canonical Fs scalar" % name)
    refused(monkeypatch, lib, [dict(a, spending_key=jj.FS_MOD, alpha=jj.FS_MOD)], "request 0: spending_key")
    refused(monkeypatch, lib, [dict(a, alpha=jj.FS_MOD, randomness=jj.FS_MOD)], "request 0: alpha")
    index_text = "s_index and t_index must be two different members of the set"
    refused(monkeypatch, lib, [dict(a, t_index=a["s_index"])], "request 0: " + index_text)
    refused(monkeypatch, lib, [b, dict(a, s_index=12)], "request 1: " + index_text)
    refused(monkeypatch, lib, [dict(a, t_index=12, spending_key=jj.FS_MOD)], "request 0: " + index_text)
    # a bad scalar goes before a bad point of the same request; a bad point of a LOWER request goes before it
    bad_point = kinds["enc_key_recipient"](a, sc.NOT_A_POINT)
    refused(monkeypatch, lib, [dict(bad_point, randomness=jj.FS_MOD)], "request 0: randomness")
    refused(monkeypatch, lib, [b, bad_point, dict(a, alpha=jj.FS_MOD)], "request 1: enc_key_recipient is not a Jubjub point")
    refused(monkeypatch, lib, [b, dict(a, alpha=jj.FS_MOD), bad_point], "request 1: alpha")


# ---------------------------------------------------------------------------------------------- arguments
def _raw_call(lib, arr, n, device=0, null=(), inputs=True):
    from zero_chain_amd import _lib
    st = (_lib.AnonymousStatement * max(n, 1))()
    rsk = C.create_string_buffer(b"\xa5" * (32 * max(n, 1)), 32 * max(n, 1))
    inp = C.create_string_buffer(104 * 32 * max(n, 1))
    args = [None if "req" in null else arr, n, device, None if "st" in null else st, None if "rsk" in null else rsk, inp if inputs else None]
    return lib.zk_anonymous_derive_dev(*args), st, rsk.raw, inp.raw


def test_arguments(lib, monkeypatch):
    import zero_chain_amd as zk
    rqs = [ad.request(0), ad.request(1)]
    arr = zk.anonymous_requests(rqs)
    for form in (HOST, DEVICE):
        monkeypatch.setenv(VAR, form)
        assert lib.zk_anonymous_derive_dev(None, 0, 0, None, None, None) == 0          # n = 0 touches nothing
        status, _, rsk, _ = _raw_call(lib, arr, 0)
        assert status == 0 and rsk == b"\xa5" * 32
        for null in ("req", "st", "rsk"):
            status, _, rsk, _ = _raw_call(lib, arr, 2, null=(null,))
            with pytest.raises(zk.ZkError) as e:
                lib.check(status)
            assert e.value.variant == "InvalidArgument" and "null argument" in str(e.value) and rsk == b"\xa5" * 64
        # inputs_out NULL: the same statements
        status, st, rsk, inp = _raw_call(lib, arr, 2)
        status_n, st_n, rsk_n, _ = _raw_call(lib, arr, 2, inputs=False)
        assert status == status_n == 0 and bytes(st) == bytes(st_n) and rsk == rsk_n
        assert zk.bytes_to_scalars(inp) == ad.expected(rqs[0])[2] + ad.expected(rqs[1])[2]
        for device in (-1, 4096):
            status, _, _, _ = _raw_call(lib, arr, 2, device=device)
            with pytest.raises(zk.ZkError) as e:
                lib.check(status)
            assert e.value.variant == "InvalidArgument" and "device index out of range" in str(e.value)
    st, rsks = zk.anonymous_derive_dev(arr, lib=lib)
    assert ad.statement_dict(st[1]) == ad.expected(rqs[1])[0] and len(rsks) == 2
    st, rsks, inputs = zk.anonymous_derive_dev(zk.anonymous_requests([]), want_inputs=True, lib=lib)
    assert (len(st), rsks, inputs) == (0, [], [])


# ---------------------------------------------------------------------------------------------- wiping, resources
def test_key_derived_device_memory_is_returned_and_wiped(lib, monkeypatch):
    """after a device-form call nothing key-derived is held, and everything released was zeroed first - also after a refusal; the
    fixed-base table - public - stays"""
    import zero_chain_amd as zk
    monkeypatch.setenv(VAR, DEVICE)
    rqs = [ad.request(0), ad.request(1)]
    zk.anonymous_derive_dev(zk.anonymous_requests(rqs[:1]), lib=lib)   # (the first kernel call of a process uploads the table: 132 096 bytes that stay)
    before = zk.memory_stats(lib=lib)
    st, rsks, inputs = zk.anonymous_derive_dev(zk.anonymous_requests(rqs), want_inputs=True, lib=lib)
    assert ad.statement_dict(st[1]) == ad.expected(rqs[1])[0]
    mid = zk.memory_stats(lib=lib)
    assert mid["device_held"] == before["device_held"] and mid["device_released"] == mid["device_wiped"]
    assert mid["device_released"] - before["device_released"] >= 2 * (12 * 64 + 5 * 32 + 17 * 128)   # the scalars and the projective points
    with pytest.raises(zk.ZkError):
        zk.anonymous_derive_dev(zk.anonymous_requests([rqs[0], dict(rqs[1], g_epoch=sc.torsion())]), lib=lib)
    after = zk.memory_stats(lib=lib)
    assert after["device_held"] == before["device_held"] and after["device_released"] == after["device_wiped"] > mid["device_released"]


def test_the_kernels_keep_their_tables_in_lds():
    """the code object's metadata: both kernels of the derived-point stage (csrc/derive_stage.h), the pair that serves this entry and
    zk_elgamal_encrypt_dev and has no per-entry sibling left - no scratch memory, LDS within the 36 864 B of k_rj_check and k_keys_points"""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    every = mod.kernel_resources(_lib.LIB_PATH)
    assert not [n for n in every if "k_anon_" in n or "k_enc_" in n]
    res = {n: r for n, r in every.items() if "k_derive_points" in n or "k_derive_combine" in n}
    assert len(res) == 2, sorted(res)
    assert all(r["scratch"] == 0 for r in res.values()), res
    assert all(r["lds"] <= 36864 for r in res.values()), res
    assert sorted(r["lds"] for r in res.values()) == [16 * 32 * 64, 17 * 32 * 64], res


# ---------------------------------------------------------------------------------------------- gen_proof
@pytest.mark.gpu
def test_gen_proof_through_both_forms(gpu_lib, monkeypatch):
    """zk_anonymous_gen_proof_batch with the derivation on the host threads and in the kernels: the same AnonymousXt, equal to the
    oracle's fields; the forced-device run launches the stage's kernels; an inconsistent request is still Unsatisfiable; and the
    public inputs of zk_anonymous_derive_dev verify the proofs zk_anonymous_prove_batch makes from its statements."""
    import zero_chain_amd as zk
    import helpers
    import test_gen_proof as tg
    cases = [tg.anonymous_request(1), tg.anonymous_request(5, amount=77, balance=5000)]
    arr = zk.anonymous_requests([c[0] for c in cases])
    rs = [(31 + i, 77 + 3 * i) for i in range(len(cases))]
    mats = zk.ConstraintMatrices.anonymous_circuit(lib=gpu_lib)
    params = pvk = None
    try:
        params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=gpu_lib)
        pvk = zk.prepare_verifying_key(params)
        monkeypatch.setenv(VAR, HOST)
        with zk.KernelTimer(gpu_lib) as t:
            host = zk.anonymous_gen_proofs(params, mats, pvk, arr, rs)
            assert [t.get(s)[0] for s in STAGES] == [0, 0]
        monkeypatch.setenv(VAR, DEVICE)
        with zk.KernelTimer(gpu_lib) as t:
            device = zk.anonymous_gen_proofs(params, mats, pvk, arr, rs)
            launches = [t.get(s)[0] for s in STAGES]
        assert launches == [1, 1], launches
        assert host == device
        for case, xt in zip(cases, device):
            want, _ = tg.anonymous_expected(*case)
            for f, v in want.items():
                assert xt[f] == v, f
        bad = dict(cases[0][0], remaining_balance=cases[0][0]["remaining_balance"] + 1)
        with pytest.raises(zk.ZkError) as e:
            zk.anonymous_gen_proofs(params, mats, pvk, zk.anonymous_requests([cases[1][0], bad]), rs)
        assert e.value.variant == "Unsatisfiable" and "request 1" in str(e.value)
        st, _, inputs = zk.anonymous_derive_dev(arr, want_inputs=True, lib=gpu_lib)
        proofs = zk.anonymous_prove_batch(mats, params, st, rs)
        assert [p.write() for p in proofs] == [xt["proof"] for xt in device]
        assert zk.verify_proofs(pvk, proofs, inputs) == [True, True]
        assert zk.verify_proofs(pvk, proofs, inputs[::-1]) == [False, False]
    finally:
        if pvk is not None:
            pvk.close()
        if params is not None:
            params.close()
        mats.close()
