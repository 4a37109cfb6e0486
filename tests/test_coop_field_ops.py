"""The wave-cooperative field of csrc/coop_field.h and the group law, import / export, exponentiation, inversion and
ordering of csrc/coop_curve.h - one Fq element over the 16 lanes of a DPP row - one function at a time, on operands whose
limbs the test chooses, against Python integers and oracle/bls12_381.py (tests/coop_cases.py), through the row ops of the
test hook zk_hook_field_op (csrc/field_hooks.cpp).  The same cases run on the x86 emulation build, where a row is an array,
the ZK_FQ28_CHECK lines are live and non-zero lanes 14 / 15 abort, and - marked gpu - on libzkamd_hooks.so, where the lane
operations are the DPP moves and the ballot of the hardware, four different rows to a wave and the last wave partial."""
import pytest

import coop_cases as cc


def test_op_table_matches_the_c_enum_and_unknown_ops_are_refused(emu_lib):
    cc.op_table_and_the_first_code_past_it(emu_lib)


def test_every_op_has_cases():
    assert len(set(cc.OP_NAMES)) == len(cc.OP_NAMES)
    for name in cc.OP_NAMES:
        assert cc.checker(name) is not None


@pytest.mark.parametrize("name", cc.OP_NAMES)
def test_op_emulated(emu_lib, name):
    assert cc.check_op(emu_lib, name) > cc.WAVE


@pytest.mark.gpu
def test_op_table_on_the_gpu(gpu_hooks_lib):
    cc.op_table_and_the_first_code_past_it(gpu_hooks_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.OP_NAMES)
def test_op_on_the_gpu(gpu_hooks_lib, name):
    n = cc.check_op(gpu_hooks_lib, name)
    assert n > cc.WAVE and n % cc.WAVE != 0      # more than one full wave of rows, and a partial one
