"""A block of confidential transfers executed in one call (tests/block_cases.py): zk_confidential_block_execute on the x86
emulation build with the kernels forced and in the host form and, under -m gpu, on the device with both settings - one set of
cases, the expected verdicts and accounts from a sequential model of the seven steps over oracle/jubjub.py; zk_g_epoch against
the oracle's group hash."""
import os

import pytest

import block_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = pytest.mark.parametrize("host_max", ["0", None], ids=["kernels", "host_form"])


def _form(monkeypatch, host_max):
    if host_max is None:
        monkeypatch.delenv("ZKAMD_INTO_XY_HOST_MAX", raising=False)
    else:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)


# ---------------------------------------------------------------------------------------------- the kernels' source, emulated
@FORMS
@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_cases_under_emulation(emu_lib, monkeypatch, host_max, name):
    _form(monkeypatch, host_max)
    bc.run_case(emu_lib, name)


@FORMS
def test_bad_arguments_under_emulation(emu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    bc.bad_arguments(emu_lib)


def test_the_case_names_are_the_cases():
    assert tuple(bc.cases()) == bc.CASE_NAMES


def test_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_INTO_XY_HOST_MAX counts the distinct encodings of a call and is read per call"""
    block = bc.cases()["honest"]
    for host_max in (block.distinct(), block.distinct() - 1):   # at it: the host form; above it: the kernels
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(host_max))
        bc.check(block, bc.execute(emu_lib, block))


def test_kernels_under_emulation_around_a_block_of_the_balance_kernel(emu_lib, monkeypatch):
    """33 extrinsics: 66 lanes of k_block_balance_xy, two in a second block"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    block = bc.all_accepted(33)
    bc.check(block, bc.execute(emu_lib, block))


def test_kernels_under_emulation_large_block(emu_lib, monkeypatch):
    """more than 256 ops by index: the scan crosses a workgroup and takes the carry; ten rejected, several rounds"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    block = bc.large_block()
    verdicts, accounts, stats = got = bc.execute(emu_lib, block)
    bc.check(block, got)
    assert sum(v[0] != "accepted" for v in verdicts) == 10 and stats["rounds"] >= 2


def test_g_epoch(emu_lib):
    bc.g_epochs(emu_lib)


def test_g_epoch_on_the_product_library():
    """zk_g_epoch runs on the host: the product library answers where no GPU is"""
    from zero_chain_amd import _lib
    bc.g_epochs(_lib.ZkLib(_lib.LIB_PATH))


def test_block_kernels_keep_their_state_in_lds():
    """The kernels as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed):
    k_block_balance_xy once, nothing in scratch memory, LDS no more than the inversion's window table (16 x 32 bytes x 64) - and
    the decoder and the ledger's three kernels still there exactly once: the block executor launches them, it compiles no copy."""
    import importlib.util
    from zero_chain_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    objects = mod.kernel_resources_per_object(_lib.LIB_PATH)
    held = lambda kernel: [r for obj in objects for n, r in obj.items() if kernel in n]
    res = held("k_block_balance_xy")
    assert len(res) == 1, res
    assert res[0]["scratch"] == 0 and 0 < res[0]["lds"] <= 16 * 32 * 64, res[0]
    res = held("k_block_gather")
    assert len(res) == 1 and res[0]["scratch"] == 0 and res[0]["lds"] == 0, res
    for kernel in ("k_into_xy", "k_ledger_scan", "k_ledger_carry", "k_ledger_encode"):
        assert len(held(kernel)) == 1, kernel


# ---------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_gpu_cases(gpu_lib, monkeypatch, host_max, name):
    _form(monkeypatch, host_max)
    bc.run_case(gpu_lib, name)


@pytest.mark.gpu
@FORMS
def test_gpu_bad_arguments_and_g_epoch(gpu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    bc.bad_arguments(gpu_lib)
    bc.g_epochs(gpu_lib)


def _both_forms(lib, monkeypatch, block):
    """the kernels, held to the model; then the same call in the host form, held to the kernels' bytes"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    on_device = bc.execute(lib, block)
    bc.check(block, on_device)
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(1 << 30))
    assert bc.execute(lib, block) == on_device
    return on_device


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_gpu_all_accepted_around_a_block_of_the_balance_kernel(gpu_lib, monkeypatch, n):
    _both_forms(gpu_lib, monkeypatch, bc.all_accepted(n))


@pytest.mark.gpu
def test_gpu_large_block_crosses_a_workgroup_of_the_scan(gpu_lib, monkeypatch):
    block = bc.large_block()
    verdicts, accounts, stats = _both_forms(gpu_lib, monkeypatch, block)
    assert sum(v[0] != "accepted" for v in verdicts) == 10 and len(verdicts) == 130
    n_ops = 3 * len(verdicts) + 2 * sum(bool(a["flags"] & bc.DUE) for a in accounts)
    assert n_ops > 256 + 64
    assert 2 <= stats["rounds"] <= 4 and stats["proofs_verified"] >= 130 - 6   # (every sender has three or four extrinsics)
