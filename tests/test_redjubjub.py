"""RedJubjub signing and the batch signature check (tests/redjubjub_cases.py): on the product library without a GPU (signing,
the host form), on the x86 emulation build (the kernels' source), the kernels' resources as built for gfx950 and, under -m gpu,
on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import redjubjub_cases as rc


@pytest.fixture(scope="module")
def host_lib():
    """the product library, opened where no GPU is: only entries that never touch the device may be called"""
    from zero_chain_amd import _lib
    return _lib.ZkLib(_lib.LIB_PATH)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_sign_gives_the_restatements_bytes(host_lib):
    import zero_chain_amd as zk
    sks = [1, 2, rc.S - 1, 0x1234567890abcdef << 120, 0]
    msgs = [b"", b"a", bytes(range(96)), bytes(200), b"Foo bar"]
    ts = [bytes((7 * i + k) & 255 for k in range(80)) for i in range(len(sks))]
    sigs = zk.redjubjub_sign(sks, ts, msgs, lib=host_lib)
    assert sigs == [rc.sign(sk, t, m) for sk, t, m in zip(sks, ts, msgs)]
    # keys as the 32 bytes the derive entries return, and the signatures verify under sk G
    assert zk.redjubjub_sign([sk.to_bytes(32, "little") for sk in sks], ts, msgs, lib=host_lib) == sigs
    vks = zk.jubjub_base_mul(sks, lib=host_lib)
    assert zk.redjubjub_verify(vks, sigs, msgs, lib=host_lib) == ([True] * len(sks), [0] * len(sks))


def test_sign_refuses_a_key_that_is_no_scalar(host_lib):
    import zero_chain_amd as zk
    keys = [(5).to_bytes(32, "little")] * 3 + [rc.S.to_bytes(32, "little")] + [(6).to_bytes(32, "little")]
    with pytest.raises(zk.ZkError) as e:
        zk.redjubjub_sign(keys, [bytes(80)] * 5, [b"m"] * 5, lib=host_lib)
    assert e.value.variant == "InvalidArgument" and "rsk 3 " in str(e.value)


def test_reference_key_pair(host_lib):
    """demo/wasm-utils/tests/web.rs:97-101: rvk = rsk G, and a signature by rsk verifies under rvk"""
    import zero_chain_amd as zk
    rsk, rvk, msg = rc.golden()
    assert zk.jubjub_base_mul([int.from_bytes(rsk, "little")], lib=host_lib) == [rvk]
    (sig,) = zk.redjubjub_sign([rsk], [bytes(range(80))], [msg], lib=host_lib)
    assert rc.verify(rvk, sig, msg) == rc.OK
    assert zk.redjubjub_verify([rvk], [sig], [msg], lib=host_lib) == ([True], [0])


def test_pool_host_form_on_the_product_library(host_lib):
    rc.verdicts_match(host_lib, rc.pool(), None)


def test_decreasing_offsets_are_refused_and_nothing_is_ok(host_lib):
    vk, sig, msg, _ = rc.pool()[1]
    two = np.frombuffer(vk + vk, dtype=np.uint8).copy(), np.frombuffer(sig + sig, dtype=np.uint8).copy(), np.frombuffer(msg + msg + b"x", dtype=np.uint8).copy()
    offs = np.array([len(msg), 2 * len(msg) + 1, len(msg)], dtype=np.uint64)
    ok = np.zeros(2, dtype=np.uint8)
    keys, ts, out = np.zeros(64, dtype=np.uint8), np.zeros(160, dtype=np.uint8), np.zeros(128, dtype=np.uint8)
    for st in (host_lib.zk_redjubjub_verify_batch(2, _ptr(two[0]), _ptr(two[1]), _ptr(two[2]), _ptr(offs), -1, _ptr(ok), None),
               host_lib.zk_redjubjub_sign(2, _ptr(keys), _ptr(ts), _ptr(two[2]), _ptr(offs), _ptr(out))):
        assert st == 16   # ZK_ERR_INVALID_ARGUMENT
        assert b"msg_offsets decrease at message 1" in host_lib.zk_last_error()
    # n = 0 touches nothing
    assert host_lib.zk_redjubjub_verify_batch(0, None, None, None, None, -1, None, None) == 0
    assert host_lib.zk_redjubjub_sign(0, None, None, None, None, None) == 0
    assert rc.raw_verify(host_lib, [], None) == (b"", b"")


@pytest.mark.parametrize("host_max", ["0", "1000000"], ids=["kernels", "host"])
def test_pool_under_emulation(emu_lib, monkeypatch, host_max):
    monkeypatch.setenv("ZKAMD_REDJUBJUB_HOST_MAX", host_max)
    rc.verdicts_match(emu_lib, rc.pool(), 0)


def test_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_REDJUBJUB_HOST_MAX is read per call; n at, below and above it give the same bytes"""
    cases = rc.pool()[61:66]   # accepted, accepted, refused, refused, accepted
    assert [c[3] == rc.OK for c in cases] == [True, True, False, False, True]
    monkeypatch.setenv("ZKAMD_REDJUBJUB_HOST_MAX", "4")
    for n in (3, 4, 5):
        ok, why = rc.raw_verify(emu_lib, cases[:n], 0)
        assert list(why) == [c[3] for c in cases[:n]] and list(ok) == [int(c[3] == rc.OK) for c in cases[:n]]


def test_kernels_keep_their_tables_in_lds():
    """The two kernels as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed): one
    of each, nothing in scratch memory, the LDS the header comment of csrc/redjubjub.h states - and k_into_xy, whose decode
    chain they share, is still one kernel."""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # per code object: kernels with internal linkage keep one mangled name in every translation unit that compiles them, so a
    # dict over the whole library would fold a second copy into the first
    objects = mod.kernel_resources_per_object(_lib.LIB_PATH)
    assert len(objects) > 1
    for name, lds in (("k_rj_decode", 16 * 32 * 64), ("k_rj_check", 18 * 32 * 64)):
        found = [r for obj in objects for n, r in obj.items() if name in n]
        assert len(found) == 1, (name, len(found))
        (r,) = found
        assert r["scratch"] == 0 and r["vgpr"] <= 256 and r["lds"] == lds, (name, r)
    assert len([n for obj in objects for n in obj if "k_into_xy" in n]) == 1
    header = open(os.path.join(root, "zero-chain_amd", "csrc", "redjubjub.h")).read()
    assert "32 768 B" in header and "36 864 B" in header


# ---------------------------------------------------------------------------------------------- on the device
FORMS = pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])


def _form(monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_REDJUBJUB_HOST_MAX", host_max)


@pytest.mark.gpu
@FORMS
def test_gpu_one_signature_at_a_time(gpu_lib, monkeypatch, host_max):
    """the whole pool at n = 1: one live lane in its block"""
    _form(monkeypatch, host_max)
    for c in rc.pool():
        rc.verdicts_match(gpu_lib, [c], 0)


@pytest.mark.gpu
@FORMS
def test_gpu_whole_pool(gpu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    rc.verdicts_match(gpu_lib, rc.pool(), 0)


@pytest.mark.gpu
@FORMS
def test_gpu_across_a_block_boundary(gpu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    rc.verdicts_match(gpu_lib, rc.pool()[:65], 0)


@pytest.mark.gpu
def test_gpu_derived_rsk_signs_for_the_statements_rvk(gpu_lib):
    """The rsk zk_transfer_derive returns signs what verifies under rvk = pgk + alpha G of the same request (host only, no proof)"""
    import zero_chain_amd as zk
    from oracle import jubjub as jj
    import test_gen_proof as tg
    rq, _ = tg.reference_request(1)
    st, rsks = zk.transfer_derive(zk.transfer_requests([rq]), lib=gpu_lib)
    g = rc.generator()
    rvk = jj.write_point(jj.add(jj.read_point(bytes(st[0].proof_generation_key)), jj.mul(g, rq["alpha"])))
    msg = b"the signed payload of an extrinsic"
    sigs = zk.redjubjub_sign(rsks, [bytes(range(80))], [msg], lib=gpu_lib)
    assert zk.redjubjub_verify([rvk], sigs, [msg], device=None, lib=gpu_lib) == ([True], [0])
    assert zk.redjubjub_verify([rvk], sigs, [msg + b"."], device=None, lib=gpu_lib) == ([False], [4])
    assert rc.verify(rvk, sigs[0], msg) == rc.OK
