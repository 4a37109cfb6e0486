"""The steps of the line preparation of B on rows (csrc/coop_verify.cpp: cv_double_step, cv_add_step with a row per point,
cvq_double_step, cvq_add_step with four rows per point) one step at a time, on operands whose limbs the test chooses, against
the formulas of pairing.h's g2_double_step / g2_add_step over Fq2 in Python integers and the group law of oracle/bls12_381.py
(tests/cv_step_cases.py), through the test hook zk_hook_cv_step.  Points on the twist inside and outside the r-torsion with
Z != 1, coordinates at the edges of the bounds the steps state for their input, the special cases that leave Z = 0 - and the
contract between this file and coop_pairing.cpp, which reads the line unreduced: the constant term below 64 p, the two
coefficients within what coop_products<4, 1> takes.  The same cases run on the x86 emulation build, where every ZK_FQ28_CHECK
bound of the steps is live, and - marked gpu - on libzkamd_hooks.so: four cases to a wave with the last wave partial for
the one-row forms, a workgroup of four rows per case for the others."""
import pytest

import cv_step_cases as cv


def test_op_table_matches_the_c_table_and_unknown_ops_are_refused(emu_lib):
    cv.op_table_and_the_first_code_past_it(emu_lib)


def test_every_op_has_cases():
    assert len(set(cv.OP_NAMES)) == len(cv.OP_NAMES) == 4
    for name in cv.OP_NAMES:
        cases, kinds = cv.build(name)
        assert {"curve", "identity", "special"} == set(kinds)
        assert name.startswith("CVQ") or len(cases) % cv.WAVE != 0


@pytest.mark.parametrize("name", cv.OP_NAMES)
def test_op_emulated(emu_lib, name):
    assert cv.check_op(emu_lib, name) >= 100


@pytest.mark.gpu
def test_op_table_on_the_gpu(gpu_hooks_lib):
    cv.op_table_and_the_first_code_past_it(gpu_hooks_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cv.OP_NAMES)
def test_op_on_the_gpu(gpu_hooks_lib, name):
    assert cv.check_op(gpu_hooks_lib, name) >= 100
