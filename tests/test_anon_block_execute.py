"""A block of anonymous transfers executed in one call (tests/anon_block_cases.py): zk_anonymous_block_execute on the x86
emulation build with the kernels forced and in the host form and, under -m gpu, on the device with both settings - one set of
cases, the expected verdicts and accounts from a sequential model of the seven steps over oracle/jubjub.py.  What the one
verification batch rests on is held in every case: rounds is never more than 1, proofs_verified is the size of the batch, and
points_decoded is the number of distinct encodings."""
import os

import pytest

import anon_block_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = pytest.mark.parametrize("host_max", ["0", None], ids=["kernels", "host_form"])


def _form(monkeypatch, host_max):
    if host_max is None:
        monkeypatch.delenv("ZKAMD_INTO_XY_HOST_MAX", raising=False)
    else:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)


def _n_ops(block, accounts):
    """twelve additions per extrinsic by index, two ops per rollover"""
    return 12 * len(block.xts) + 2 * sum(bool(a["flags"] & ac.ROLLED) for a in accounts)


# ---------------------------------------------------------------------------------------------- the kernels' source, emulated
@FORMS
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_cases_under_emulation(emu_lib, monkeypatch, host_max, name):
    _form(monkeypatch, host_max)
    ac.run_case(emu_lib, name)


@FORMS
def test_bad_arguments_under_emulation(emu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    ac.bad_arguments(emu_lib)


def test_the_case_names_are_the_cases():
    assert tuple(ac.cases()) == ac.CASE_NAMES


def test_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_INTO_XY_HOST_MAX counts the distinct encodings of a call and is read per call"""
    block = ac.cases()["honest"]
    for host_max in (block.distinct(), block.distinct() - 1):   # at it: the host form; above it: the kernels
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(host_max))
        ac.check(block, ac.execute(emu_lib, block))


def test_the_one_call_decodes_each_distinct_encoding_once():
    """27 per extrinsic, four per account and g_epoch where nothing recurs; the honest block's rings overlap, and its count is
    below the 51 n + 1 points the verifier entry decodes alone"""
    block = ac.rolled_accounts(1)
    assert block.distinct() == 3 * (27 - 12) + 36 * 5 + 1   # (the twelve keys of a ring are its accounts' keys)
    honest = ac.cases()["honest"]
    assert honest.distinct() < 51 * len(honest.xts) + 1


@pytest.mark.parametrize("r", [1, 33])
def test_kernels_under_emulation_rolled_accounts(emu_lib, monkeypatch, r):
    """2 r lanes of k_ring_balance_xy: one block not full, and two lanes in a second block"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    block = ac.rolled_accounts(r)
    ac.check(block, ac.execute(emu_lib, block))


def test_kernels_under_emulation_rows_around_a_block_of_the_gather(emu_lib, monkeypatch):
    """5 extrinsics to verify: 260 row lanes, four in a second 256-lane block"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    block = ac.to_verify(5)
    ac.check(block, ac.execute(emu_lib, block))


def test_kernels_under_emulation_large_block(emu_lib, monkeypatch):
    """more than 256 + 64 ops by index: the scan crosses a workgroup and takes the carry; six rejected for mixed reasons"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    block = ac.large_block()
    verdicts, accounts, stats = got = ac.execute(emu_lib, block)
    ac.check(block, got)
    assert sum(v[0] != "accepted" for v in verdicts) == ac.LARGE_REJECTED and len(verdicts) == ac.LARGE_N
    assert 12 * ac.LARGE_N == 360 and _n_ops(block, accounts) > 256 + 64


def test_ring_kernel_keeps_its_state_in_lds():
    """The kernels as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed):
    k_ring_balance_xy once, nothing in scratch memory, LDS no more than the inversion's window table (16 x 32 bytes x 64).  The
    input rows are k_block_gather's copies (the table of rolled balances lies behind the decoded points, on the
    same base), so that kernel is the row kernel: once, no LDS, no scratch.  The decoder, the confidential balance kernel and the
    ledger's three kernels are still there exactly once: the executor launches them, it compiles no copy."""
    import importlib.util
    from zero_chain_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    objects = mod.kernel_resources_per_object(_lib.LIB_PATH)
    held = lambda kernel: [r for obj in objects for n, r in obj.items() if kernel in n]
    res = held("k_ring_balance_xy")
    assert len(res) == 1, res
    assert res[0]["scratch"] == 0 and 0 < res[0]["lds"] <= 16 * 32 * 64, res[0]
    assert len(held("k_ring_")) == 1   # (no other new kernel)
    res = held("k_block_gather")
    assert len(res) == 1 and res[0]["scratch"] == 0 and res[0]["lds"] == 0, res
    for kernel in ("k_block_balance_xy", "k_into_xy", "k_ledger_scan", "k_ledger_carry", "k_ledger_encode"):
        assert len(held(kernel)) == 1, kernel


# ---------------------------------------------------------------------------------------------- on the device
def _both_forms(lib, monkeypatch, block):
    """the kernels, held to the model; then the same call in the host form, held to the kernels' bytes"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    on_device = ac.execute(lib, block)
    ac.check(block, on_device)
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(1 << 30))
    assert ac.execute(lib, block) == on_device
    return on_device


@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_gpu_cases(gpu_lib, monkeypatch, name):
    _both_forms(gpu_lib, monkeypatch, ac.cases()[name])


@pytest.mark.gpu
@FORMS
def test_gpu_bad_arguments(gpu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    ac.bad_arguments(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 31, 32, 33])
def test_gpu_rolled_accounts_around_a_block_of_the_balance_kernel(gpu_lib, monkeypatch, r):
    """2 r = 2 / 62 / 64 / 66 lanes of k_ring_balance_xy"""
    _both_forms(gpu_lib, monkeypatch, ac.rolled_accounts(r))


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [4, 5])
def test_gpu_rows_around_a_block_of_the_gather(gpu_lib, monkeypatch, nv):
    """52 nv = 208 / 260 row lanes, around a 256-lane block"""
    _both_forms(gpu_lib, monkeypatch, ac.to_verify(nv))


@pytest.mark.gpu
def test_gpu_large_block_crosses_a_workgroup_of_the_scan(gpu_lib, monkeypatch):
    block = ac.large_block()
    verdicts, accounts, stats = _both_forms(gpu_lib, monkeypatch, block)
    assert sum(v[0] != "accepted" for v in verdicts) == ac.LARGE_REJECTED and len(verdicts) == ac.LARGE_N
    assert 12 * ac.LARGE_N == 360 and _n_ops(block, accounts) > 256 + 64
