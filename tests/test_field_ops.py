"""Every field operation of csrc/dev_field.h and the XYZZ group law of csrc/dev_curve.h, one at a time, on operands whose
limbs the test chooses, against Python integers and oracle/bls12_381.py (tests/field_cases.py), through the test hook
zk_hook_field_op (csrc/field_hooks.cpp).  The same cases run on the x86 emulation build, whose products are the plain C++
of the column schedule and whose ZK_FQ28_CHECK lines are live, and - marked gpu - on libzkamd_hooks.so, where the products are
the assembly routines of mul_asm.h as the hardware executes them, 64 different rows to a wave and the last wave partial."""
import pytest

import field_cases as fc


def test_op_table_matches_the_c_enum_and_unknown_ops_are_refused(emu_lib):
    fc.op_table_and_the_first_code_past_it(emu_lib)


def test_every_op_has_cases():
    assert len(set(fc.OP_NAMES)) == len(fc.OP_NAMES)
    for name in fc.OP_NAMES:
        assert fc.checker(name) is not None


@pytest.mark.parametrize("name", fc.OP_NAMES)
def test_op_emulated(emu_lib, name):
    assert fc.check_op(emu_lib, name) > 64


@pytest.mark.gpu
def test_op_table_on_the_gpu(gpu_hooks_lib):
    fc.op_table_and_the_first_code_past_it(gpu_hooks_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.OP_NAMES)
def test_op_on_the_gpu(gpu_hooks_lib, name):
    assert fc.check_op(gpu_hooks_lib, name) > 64      # at least one full wave and a partial one
