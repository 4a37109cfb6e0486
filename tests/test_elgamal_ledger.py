"""A block's ElGamal balance updates as a segmented sum (tests/ledger_cases.py): zk_elgamal_ledger_apply on the product library
without a GPU (host form), on the x86 emulation build (the kernels' source) and, under -m gpu, on the device - one set of
cases, the expected values from a sequential model over oracle/jubjub.py."""
import os
import re

import pytest

import ledger_cases as lc
import xt_verify_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(lc.cases())


@pytest.fixture(scope="module")
def host_lib():
    """the product library, opened where no GPU is: only entries that never touch the device may be called"""
    from zero_chain_amd import _lib
    return _lib.ZkLib(_lib.LIB_PATH)


@pytest.fixture
def kernels(monkeypatch):
    """every call takes the device form, whatever it holds"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")


def test_the_scan_width_python_states_is_the_source_s():
    src = open(os.path.join(ROOT, "zero-chain_amd", "csrc", "ledger.h")).read()
    assert int(re.search(r"constexpr uint32_t LEDGER_SCAN_W = (\d+);", src).group(1)) == lc.W
    assert lc.W >= 128 and lc.W & (lc.W - 1) == 0   # (the cases place ops around lane 64 and around W)


# ---------------------------------------------------------------------------------------------- the host form, no GPU
@pytest.mark.parametrize("name", CASES)
def test_host_form(host_lib, name):
    lc.run_case(host_lib, None, name)


def test_host_form_nothing_to_do(host_lib):
    lc.nothing_to_do(host_lib, None)


def test_host_form_bad_arguments(host_lib):
    lc.bad_arguments(host_lib, None)


def test_host_form_mirror(host_lib):
    lc.mirror(host_lib, None)


def test_host_form_against_elgamal_add(host_lib):
    lc.against_elgamal_add(host_lib, None)


# ---------------------------------------------------------------------------------------------- the kernels' source, emulated
@pytest.mark.parametrize("name", CASES)
def test_kernels_under_emulation(emu_lib, kernels, name):
    lc.run_case(emu_lib, 0, name)


def test_kernels_under_emulation_nothing_to_do(emu_lib, kernels):
    lc.nothing_to_do(emu_lib, 0)


def test_kernels_under_emulation_bad_arguments(emu_lib, kernels):
    lc.bad_arguments(emu_lib, 0)


def test_kernels_under_emulation_mirror(emu_lib, kernels):
    lc.mirror(emu_lib, 0)


def test_kernels_under_emulation_against_elgamal_add(emu_lib, kernels):
    lc.against_elgamal_add(emu_lib, 0)


def test_tails_in_two_passes_under_emulation(emu_lib, kernels):
    lc.tails_in_two_passes(emu_lib, 0)


def test_two_transfers_from_one_sender_under_emulation(emu_lib, kernels):
    lc.two_transfers_from_one_sender(emu_lib, 0)


def test_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_INTO_XY_HOST_MAX counts the points of a call, 2 (n_slots + n_ops), and is read per call: a call at, below and
    above it gives the same bytes"""
    slots, ops = lc.cases()["refused_slot_1"]   # 3 slots, 7 ops: 20 points
    want = lc.model(list(slots), list(ops))
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(2 * (3 + 6)))
    for n in (6, 7):   # n = 6 sits at it (the host form), n = 7 above it (the kernels)
        assert lc.raw_apply(emu_lib, list(slots), list(ops[:n]), 0)[1:] == lc.model(list(slots), list(ops[:n]))
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "21")   # below it
    assert lc.raw_apply(emu_lib, list(slots), list(ops), 0)[1:] == want
    monkeypatch.delenv("ZKAMD_INTO_XY_HOST_MAX")
    assert lc.raw_apply(emu_lib, list(slots), list(ops), 0)[1:] == want


def test_ledger_kernels_keep_their_state_in_lds():
    """The kernels as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed): each
    new kernel once, nothing in scratch memory, LDS no more than DESIGN.md 4.9 states - one EP per lane of the scan (4 x 32
    bytes x W), the inversion's window table in the encoder (16 x 32 bytes x 64) - and k_into_xy still there exactly once."""
    import importlib.util
    from zero_chain_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    objects = mod.kernel_resources_per_object(_lib.LIB_PATH)   # (per code object: a kernel two units compile is counted twice)
    held = lambda kernel: [r for obj in objects for n, r in obj.items() if kernel in n]
    for kernel, lds in (("k_ledger_scan", 4 * 32 * lc.W), ("k_ledger_carry", 4 * 32 * lc.W), ("k_ledger_encode", 16 * 32 * 64)):
        res = held(kernel)
        assert len(res) == 1, (kernel, res)
        assert res[0]["scratch"] == 0 and 0 < res[0]["lds"] <= lds, (kernel, res[0])
    assert len(held("k_into_xy")) == 1


# ---------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernels", "default"])
@pytest.mark.parametrize("name", CASES)
def test_gpu_cases(gpu_lib, monkeypatch, host_max, name):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    lc.run_case(gpu_lib, 0, name)


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernels", "default"])
def test_gpu_arguments_mirror_and_elgamal_add(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    lc.nothing_to_do(gpu_lib, 0)
    lc.bad_arguments(gpu_lib, 0)
    lc.mirror(gpu_lib, 0)
    lc.against_elgamal_add(gpu_lib, 0)


@pytest.mark.gpu
def test_gpu_tails_in_two_passes(gpu_lib):
    lc.tails_in_two_passes(gpu_lib, 0)   # (far above the threshold: the default is the kernels)


@pytest.mark.gpu
@pytest.mark.parametrize("host_max", ["0", None], ids=["kernels", "default"])
def test_gpu_two_transfers_from_one_sender(gpu_lib, monkeypatch, host_max):
    if host_max is not None:
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", host_max)
    lc.two_transfers_from_one_sender(gpu_lib, 0)
