"""A block of encrypted-asset extrinsics executed in one call (tests/asset_block_cases.py): zk_asset_block_execute on the x86
emulation build with the kernels forced and in the host form and, under -m gpu, on the device with the kernels held to the model
and the host form held to the kernels' bytes - one set of cases, the expected verdicts, accounts, effects and ids from a
sequential model of the three step lists over oracle/jubjub.py."""
import os
import subprocess

import pytest

import asset_block_cases as ac
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
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_cases_under_emulation(emu_lib, monkeypatch, host_max, name):
    _form(monkeypatch, host_max)
    ac.run_case(emu_lib, name)


def test_the_case_names_are_the_cases():
    assert tuple(ac.cases()) == ac.CASE_NAMES


@FORMS
@pytest.mark.parametrize("name", ["honest", "one_sender_twice_both_valid", "same_nonce_first_accepted", "refused_fields_torsion", "unreadable_accounts"])
def test_a_transfer_only_block_is_the_confidential_entry_s_under_emulation(emu_lib, monkeypatch, host_max, name):
    _form(monkeypatch, host_max)
    ac.equals_the_confidential_entry(emu_lib, bc.cases()[name])


@FORMS
def test_bad_arguments_under_emulation(emu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    ac.bad_arguments(emu_lib)


@FORMS
def test_the_split_recourse_under_emulation(emu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    ac.split_recourse(emu_lib)


def test_forms_meet_at_the_threshold(emu_lib, monkeypatch):
    """ZKAMD_INTO_XY_HOST_MAX counts the distinct encodings of a call and is read per call"""
    block = ac.cases()["honest_mixed"]
    for host_max in (block.distinct(), block.distinct() - 1):   # at it: the host form; above it: the kernels
        monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(host_max))
        ac.check(block, ac.execute(emu_lib, block))


def _both_forms(lib, monkeypatch, block):
    """the kernels, held to the model; then the same call in the host form, held to the kernels' bytes"""
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    on_device = ac.execute(lib, block)
    ac.check(block, on_device)
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", str(1 << 30))
    assert ac.execute(lib, block) == on_device
    return on_device


def test_kernels_under_emulation_around_a_block_of_the_balance_kernel(emu_lib, monkeypatch):
    """33 rows: 66 lanes of k_asset_balance_xy, the last pair - a destroy's - in a second block and left alone"""
    _both_forms(emu_lib, monkeypatch, ac.rows(33))


def test_kernels_under_emulation_encode_outputs_around_64(emu_lib, monkeypatch):
    _both_forms(emu_lib, monkeypatch, ac.encode_outputs(16, 1))   # 68 outputs: the destroy's four in a second block


def test_kernels_under_emulation_large_block(emu_lib, monkeypatch):
    """more than 256 + 64 ops: the scan crosses a workgroup with a destroy on each side of the boundary; several rounds"""
    block = ac.large_block()
    verdicts, accounts, effects, next_id, stats = _both_forms(emu_lib, monkeypatch, block)
    _large_block_is_what_it_says(block, verdicts, accounts, stats)


def _large_block_is_what_it_says(block, verdicts, accounts, stats):
    W = 256
    n_transfers, n_destroys = block.kinds.count("transfer"), block.kinds.count("destroy")
    rolls = {(block.ids[i], block.xts[i][f]) for i, k in enumerate(block.kinds) if k == "transfer" for f in ("enc_key_sender", "enc_key_recipient")}
    n_ops = 3 * n_transfers + 2 * n_destroys + 2 * sum(bool(a["flags"] & ac.DUE) and (a["asset_id"], a["enc_key"]) in rolls for a in accounts)
    assert n_ops > W + 64 and stats["rounds"] >= 2
    # the slots of account k begin, in slot-major order, behind the ops of the accounts before it: destroyed accounts on either side of place W
    accepted = [k for k, a in enumerate(accounts) if a["flags"] & ac.TAKEN]
    assert min(accepted) < 10 and max(accepted) > 30 and len(accepted) >= 6


# ---------------------------------------------------------------------------------------------- the ABI and the code objects
def test_the_effect_is_136_bytes_in_c(tmp_path):
    """zk_asset_effect as a C compiler lays it out, against the ctypes mirror"""
    import ctypes as C
    from zero_chain_amd import _lib
    src = tmp_path / "effect.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkamd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u %d", sizeof(zk_asset_effect), offsetof(zk_asset_effect, first), offsetof(zk_asset_effect, second), '
                   'offsetof(zk_asset_effect, reserved), ZK_BLOCK_TAKEN, ZK_ASSET_TRANSFER + 10 * ZK_ASSET_ISSUE + 100 * ZK_ASSET_DESTROY); return 0; }\n')
    exe = tmp_path / "effect"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split()
    E = _lib.AssetEffect
    assert got == [str(v) for v in (C.sizeof(E), E.first.offset, E.second.offset, E.reserved.offset, ac.TAKEN, 210)]
    assert C.sizeof(E) == 136 and ac.zk.ASSET_KINDS == ("transfer", "issue", "destroy")


def test_asset_kernels_keep_their_state_in_lds():
    """The kernels as built for gfx950 (tools/kernel_resources.py reads the code objects of the library; no GPU needed): each of
    the four new kernels once, nothing in scratch memory, scan and carry within one EP and one word per lane of LDS, the two
    consumers within the inversion's window table - and the six kernels the executor launches but does not copy still once."""
    import importlib.util
    from zero_chain_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    objects = mod.kernel_resources_per_object(_lib.LIB_PATH)
    held = lambda kernel: [r for obj in objects for n, r in obj.items() if kernel in n]
    W = 256
    for kernel, lds in (("k_asset_scan", 4 * 32 * W + 4 * W), ("k_asset_carry", 4 * 32 * W + 4 * W), ("k_asset_encode", 16 * 32 * 64), ("k_asset_balance_xy", 16 * 32 * 64)):
        res = held(kernel)
        assert len(res) == 1, (kernel, res)
        assert res[0]["scratch"] == 0 and 0 < res[0]["lds"] <= lds, (kernel, res[0])
    for kernel in ("k_ledger_scan", "k_ledger_carry", "k_ledger_encode", "k_block_balance_xy", "k_block_gather", "k_into_xy"):
        assert len(held(kernel)) == 1, kernel
    assert len(held("k_ring_")) == 1


# ---------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_gpu_cases(gpu_lib, monkeypatch, name):
    _both_forms(gpu_lib, monkeypatch, ac.cases()[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["honest", "one_sender_twice_both_valid"])
def test_gpu_a_transfer_only_block_is_the_confidential_entry_s(gpu_lib, monkeypatch, name):
    monkeypatch.setenv("ZKAMD_INTO_XY_HOST_MAX", "0")
    ac.equals_the_confidential_entry(gpu_lib, bc.cases()[name])


@pytest.mark.gpu
@FORMS
def test_gpu_bad_arguments_and_the_split_recourse(gpu_lib, monkeypatch, host_max):
    _form(monkeypatch, host_max)
    ac.bad_arguments(gpu_lib)
    ac.split_recourse(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [31, 32, 33])
def test_gpu_rows_around_a_block_of_the_balance_kernel(gpu_lib, monkeypatch, nv):
    _both_forms(gpu_lib, monkeypatch, ac.rows(nv))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(15, 1), (16, 0), (16, 1)], ids=["64", "64_no_destroy", "68"])
def test_gpu_encode_outputs_around_64(gpu_lib, monkeypatch, shape):
    _both_forms(gpu_lib, monkeypatch, ac.encode_outputs(*shape))


@pytest.mark.gpu
def test_gpu_large_block_crosses_a_workgroup_of_the_scan(gpu_lib, monkeypatch):
    block = ac.large_block()
    verdicts, accounts, effects, next_id, stats = _both_forms(gpu_lib, monkeypatch, block)
    _large_block_is_what_it_says(block, verdicts, accounts, stats)
