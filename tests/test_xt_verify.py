"""Transfer extrinsics from their bytes (tests/xt_verify_cases.py): IntoXY and the two transaction entries on the product
library without a GPU (host form), on the x86 emulation build (the kernel's source) and, under -m gpu, on the device."""
import os

import pytest

import helpers
import xt_verify_cases as xc


@pytest.fixture(scope="module")
def host_lib():
    """the product library, opened where no GPU is: only entries that never touch the device may be called"""
    from zero_chain_amd import _lib
    return _lib.ZkLib(_lib.LIB_PATH)


def test_into_xy_host_form_on_the_product_library(host_lib):
    xc.into_xy_against_oracle(host_lib, None)


def test_into_xy_kernel_under_emulation(emu_lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    xc.into_xy_against_oracle(emu_lib, 0)


def test_into_xy_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_INTO_XY_HOST_MAX is read per call; n at, below and above it give the same bytes"""
    good, bad = xc.pool()
    encs = [good[5], bad[1], good[6], bad[2], good[7]]
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "4")
    want = [xc.expected(e) for e in encs]
    for n in (3, 4, 5):
        xy, st = xc.raw_into_xy(emu_lib, encs[:n], 0)
        assert st == [w[0] for w in want[:n]] and xy == b"".join(w[1] for w in want[:n])
    monkeypatch.delenv("ZKAMD_INTO_XY_HOST_MAX")
    xy, st = xc.raw_into_xy(emu_lib, encs, 0)
    assert st == [w[0] for w in want] and xy == b"".join(w[1] for w in want)


def test_confidential_verdicts_under_emulation(emu_lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    xc.confidential_verdicts(emu_lib)


def test_confidential_verdicts_host_form_under_emulation(emu_lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "1000000")
    xc.confidential_verdicts(emu_lib)


def test_anonymous_verdicts_under_emulation(emu_lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    xc.anonymous_verdicts(emu_lib)


def test_reference_vector_under_emulation(emu_lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    xc.reference_vector(emu_lib)


def test_into_xy_kernel_keeps_its_tables_in_lds():
    """The kernel as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed): the two
    window tables live in LDS - 16 slots x 32 bytes x 64 lanes - and nothing in scratch memory, at one wave per block."""
    import importlib.util
    from zero_chain_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources(_lib.LIB_PATH).items() if "k_into_xy" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["scratch"] == 0 and r["lds"] == 16 * 32 * 64 and r["vgpr"] <= 256, r


# ---------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])
def test_gpu_into_xy(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    xc.into_xy_against_oracle(gpu_lib, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])
def test_gpu_confidential_verdicts(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    xc.confidential_verdicts(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])
def test_gpu_anonymous_verdicts(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    xc.anonymous_verdicts(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])
def test_gpu_reference_vector(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    xc.reference_vector(gpu_lib)


def _flip_nonce(xt):
    b = bytearray(xt["nonce"])
    b[0] ^= 1
    return dict(xt, nonce=bytes(b))


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernel", "default"])
def test_gpu_generated_confidential_xts_are_accepted(gpu_lib, monkeypatch, host_max):
    """Three transactions from zk_transfer_gen_proof_batch under helpers.transfer_case's key go through the new entry from
    their bytes alone (enc_balances = NULL: each xt's own field); with one bit of the nonce flipped they do not."""
    import zero_chain_amd as zk
    from oracle import gen_proof as og
    from oracle import jubjub as jj
    import test_gen_proof as tg
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    r1, asgs, P, pk = helpers.transfer_case(1)
    items = []
    for k in range(3):
        rq, bal = tg.reference_request(k + 1)
        if k:
            sk = og.spending_key_from_seed(b"sender %d" % k)
            _, _, ek = og.derive(sk)
            bal = og.encrypt(500 + k, 7 + k, ek)
            rq.update(spending_key=sk, amount=20 + k, fee=k, remaining_balance=500 + k - 20 - k - k,
                      enc_balance_left=jj.write_point(bal[0]), enc_balance_right=jj.write_point(bal[1]))
        items.append(rq)
    rs = [(11 + i, 23 + 5 * i) for i in range(len(items))]
    params = zk.Parameters.read(pk, checked=False, lib=gpu_lib)
    mats = zk.ConstraintMatrices.transfer_circuit(lib=gpu_lib)
    pvk = zk.prepare_verifying_key(params)
    try:
        raw = zk.gen_proofs(params, mats, pvk, zk.transfer_requests(items), rs, raw=True)
        epochs = [rq["g_epoch"] for rq in items]
        assert zk.verify_confidential_xts(pvk, raw, epochs) == ([True] * 3, [None] * 3)
        assert zk.verify_confidential_xts(pvk, raw, epochs[0]) == ([True] * 3, [None] * 3)   # (the three share the epoch)
        assert len(set(epochs)) == 1
        xts = [zk.xt_fields(x) for x in raw]
        ok, ref = zk.verify_confidential_xts(pvk, [_flip_nonce(x) for x in xts], epochs)
        assert ok == [False] * 3
        ok, ref = zk.verify_confidential_xts(pvk, [xts[0], _flip_nonce(xts[1]), xts[2]], epochs)
        assert ok == [True, False, True]
    finally:
        pvk.close()
        mats.close()
        params.close()


@pytest.mark.gpu
def test_gpu_generated_anonymous_xt_is_accepted(gpu_lib, monkeypatch):
    """One transaction from zk_anonymous_gen_proof_batch is accepted from its bytes and the set members' stored balances;
    with one bit of the nonce flipped it is not."""
    import zero_chain_amd as zk
    import test_gen_proof as tg
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    rq = tg.anonymous_request(1)[0]
    mats = zk.ConstraintMatrices.anonymous_circuit(lib=gpu_lib)
    params = pvk = None
    try:
        params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=gpu_lib)
        pvk = zk.prepare_verifying_key(params)
        (xt,) = zk.anonymous_gen_proofs(params, mats, pvk, zk.anonymous_requests([rq]), [(31, 77)])
        bal = [list(zip(rq["enc_balances_left"], rq["enc_balances_right"]))]
        assert zk.verify_anonymous_xts(pvk, [xt], rq["g_epoch"], bal) == ([True], [None])
        ok, ref = zk.verify_anonymous_xts(pvk, [xt, _flip_nonce(xt)], [rq["g_epoch"]] * 2, bal * 2)
        assert ok == [True, False]
    finally:
        if pvk is not None:
            pvk.close()
        if params is not None:
            params.close()
        mats.close()
