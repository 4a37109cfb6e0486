"""The Fq12 arithmetic of the verifier's row path (csrc/coop_pairing.cpp: an Fq12 value on TWELVE rows, a product one
accumulator of up to twelve terms) one function at a time, on operands whose limbs the test chooses, against Python integers
(tests/c12_cases.py), through the test hook zk_hook_c12_op: c12_mul (and its use as a square and after c12_conj), c12_line,
c12_cyc_sqr, c12_mul_fq2 for j = 0, 1, 2, c12_conj, c12_exp_x, c12_inv and the word order of c12_pos.  coop_products checks
neither the sum of its terms nor the width of its columns, so the magnitude arguments in that file's comments are checked
here: the operands reach the bounds the comments state, in every limb form, and every output row must be weakly normalised,
below its stated bound and exactly the reference's residue.  The same cases run on the x86 emulation build, where the
ZK_FQ28_CHECK lines of the linear operations are live, and - marked gpu - on libzkamd_hooks.so, twelve rows to a workgroup."""
import pytest

import c12_cases as c12


def test_reference_agrees_with_the_oracle():
    c12.reference_agrees_with_the_oracle()
    assert c12.frobenius_is_validated()


def test_op_table_matches_the_c_table_and_unknown_ops_are_refused(emu_lib):
    c12.op_table_and_the_first_code_past_it(emu_lib)


def test_every_op_has_cases():
    assert len(set(c12.OP_NAMES)) == len(c12.OP_NAMES)
    for name in c12.OP_NAMES:
        assert c12.checker(name) is not None


@pytest.mark.parametrize("name", c12.OP_NAMES)
def test_op_emulated(emu_lib, name):
    assert c12.check_op(emu_lib, name) >= 40


@pytest.mark.gpu
def test_op_table_on_the_gpu(gpu_hooks_lib):
    c12.op_table_and_the_first_code_past_it(gpu_hooks_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", c12.OP_NAMES)
def test_op_on_the_gpu(gpu_hooks_lib, name):
    assert c12.check_op(gpu_hooks_lib, name) >= 40


def test_the_hooks_exist_only_under_zk_test_hooks():
    """zk_hook_c12_op, zk_hook_cv_step and their kernels are named only inside #ifdef ZK_TEST_HOOKS blocks of the two units, and
    the built libraries agree: the shipped one carries neither entry, the hooks library both."""
    import os
    from zero_chain_amd import _lib
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zero-chain_amd", "csrc")
    names = ("zk_hook_c12_op", "k_c12_op", "ZK_HK_C12_OPS", "zk_hook_cv_step", "k_cv_test_step", "k_cvq_test_step", "ZK_HK_CV_OPS")
    inside_total = 0
    for unit in ("coop_pairing.cpp", "coop_verify.cpp"):
        stack = []                                           # one entry per open conditional: is it #ifdef ZK_TEST_HOOKS
        for line in open(os.path.join(csrc, unit)):
            t = line.strip()
            if t.startswith(("#ifdef", "#ifndef", "#if ")):
                stack.append(t.split()[:2] == ["#ifdef", "ZK_TEST_HOOKS"])
            elif t.startswith("#endif"):
                stack.pop()
            elif any(n in line for n in names):
                assert any(stack), (unit, line)
                inside_total += 1
        assert not stack, unit
    assert inside_total >= len(names)
    if os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOOKS_LIB_PATH):
        shipped, hooks = open(_lib.LIB_PATH, "rb").read(), open(_lib.HOOKS_LIB_PATH, "rb").read()
        for name in (b"zk_hook_c12_op", b"zk_hook_cv_step", b"k_c12_op", b"k_cv_test_step"):
            assert name not in shipped and name in hooks, name
