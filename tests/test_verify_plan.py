"""The plan of one chunk of a verification (csrc/verify_plan.h) pinned without a GPU, through the test hook
zk_hook_verify_plan of the emulation build: (a) the default forms on both sides of every threshold, (b) each of the eight
environment variables moves the fields it names and no other, (c) ZKAMD_VERIFY_WIDE=0.

Every form gives the same verdicts (parity_cases.verifier_forms_agree holds them to that), so a threshold that moves by
accident passes every verdict test and only changes what a block of transfers costs: this file sees it.  The expected values
are literals read off the launch sequence of verify_chunk / verify_batch / zk_proof_read_batch as it stood before the plan
was split out of it, never the output of verify_plan.h."""
import ctypes as C

import pytest

# the order of the words zk_hook_verify_plan returns (csrc/verify.cpp)
FIELDS = "decode b_torsion_in_decoder subgroup_tests prepare prep_b_points inputs inputs_mul pairing combined".split()
TUNABLES = ("ZKAMD_VERIFY_WIDE", "ZKAMD_COOP_VERIFY", "ZKAMD_COOP_PAIRING", "ZKAMD_INPUTS_WINDOWS", "ZKAMD_COOP_INPUTS_MAX",
            "ZKAMD_COOP_PAIRING_MAX", "ZKAMD_INPUTS_FINE_MIN", "ZKAMD_VERIFY_RLC_MIN")
NONE, ROWS, LANES = 0, 1, 2                 # decode; prepare: NONE, ROWS, TRI (k_g2_prepare_tri)
TRI = 2
IN_ROWS, WINDOWS, SIXTEEN, FOUR = 0, 1, 2, 3
P_ROWS, LANES18, THREAD = 0, 1, 2
PER_PROOF, COMBINED, AUTO = 0, 1, 2         # csrc/host_common.h VerifyForm


@pytest.fixture(autouse=True)
def _no_tunables(monkeypatch):
    for name in TUNABLES:
        monkeypatch.delenv(name, raising=False)


def plan(lib, n, n_inputs=4, own=False, affine=False, form=PER_PROOF):
    fn = lib.dll.zk_hook_verify_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_size_t]
    out = (C.c_uint64 * len(FIELDS))()
    lib.check(fn(n, n_inputs, int(own), int(affine), form, out, len(out)))
    return dict(zip(FIELDS, out))


def stages(d):
    return d["decode"], d["prepare"], d["inputs"], d["pairing"]


def changed(a, b):
    return {k for k in FIELDS if a[k] != b[k]}


def want(decode, b_torsion, tests, prepare, prep_b, inputs, mul, pairing, combined=0):
    """tests: the subgroup tests of a foreign byte string - the decoder of A and C runs theirs, the line preparation gets B's
    state words (own_proofs ? 0 : 1 and own_proofs ? null : st_g2 in the launch sequence this was read off)"""
    return dict(zip(FIELDS, (decode, b_torsion, tests, prepare, prep_b, inputs, mul, pairing, combined)))


# ------------------------------------------------------------------------------------------------------------------------
# (a) the defaults: rows for everything up to 64 proofs, for everything but the input accumulator up to 2048, lanes beyond;
# the one-lane accumulator in four pieces below 256 proofs, over the window table (no inputs: sixteen pieces) from 256
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, with_inputs, without_inputs", [
    (1, IN_ROWS, IN_ROWS), (64, IN_ROWS, IN_ROWS), (65, FOUR, FOUR), (255, FOUR, FOUR), (256, WINDOWS, SIXTEEN), (2048, WINDOWS, SIXTEEN)])
def test_default_forms_up_to_2048_proofs(emu_lib, n, with_inputs, without_inputs):
    assert plan(emu_lib, n) == want(ROWS, 0, 1, ROWS, 0, with_inputs, 1, P_ROWS)
    assert plan(emu_lib, n, n_inputs=0) == want(ROWS, 0, 1, ROWS, 0, without_inputs, 0, P_ROWS)


@pytest.mark.parametrize("n", [2049, 8192])
def test_default_forms_beyond_2048_proofs(emu_lib, n):
    assert plan(emu_lib, n) == want(LANES, 0, 1, TRI, n, WINDOWS, 1, LANES18)
    assert plan(emu_lib, n, n_inputs=0) == want(LANES, 0, 1, TRI, n, SIXTEEN, 0, LANES18)


@pytest.mark.parametrize("n", [1, 16])
def test_own_proofs_with_and_without_the_affine_hand_over(emu_lib, n):
    # no r-torsion test anywhere (decoder of A and C, state words of the preparation); with the coordinates: no decoder
    assert plan(emu_lib, n, own=True) == want(ROWS, 0, 0, ROWS, 0, IN_ROWS, 1, P_ROWS)
    assert plan(emu_lib, n, own=True, affine=True) == want(NONE, 0, 0, ROWS, 0, IN_ROWS, 1, P_ROWS)
    # coordinates without own_proofs are not looked at (verify_chunk drops the pointer)
    assert plan(emu_lib, n, affine=True) == plan(emu_lib, n)


def test_own_proofs_beyond_the_rows(emu_lib):
    assert plan(emu_lib, 2049, own=True) == want(LANES, 0, 0, TRI, 2049, WINDOWS, 1, LANES18)
    assert plan(emu_lib, 2049, own=True, affine=True) == want(NONE, 0, 0, TRI, 2049, WINDOWS, 1, LANES18)


def test_combined_check_from_4096_proofs_or_on_request_from_8(emu_lib):
    assert [plan(emu_lib, n, form=AUTO)["combined"] for n in (8, 4095, 4096, 8192)] == [0, 0, 1, 1]
    assert [plan(emu_lib, n, form=COMBINED)["combined"] for n in (1, 7, 8, 8192)] == [0, 0, 1, 1]
    assert [plan(emu_lib, n, form=PER_PROOF)["combined"] for n in (7, 8, 4096, 8192)] == [0, 0, 0, 0]
    # ... and nothing else hangs on the form
    assert changed(plan(emu_lib, 4096, form=AUTO), plan(emu_lib, 4096, form=PER_PROOF)) == {"combined"}


# ------------------------------------------------------------------------------------------------------------------------
# (b) the eight variables
# ------------------------------------------------------------------------------------------------------------------------
def test_coop_verify_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 16)
    monkeypatch.setenv("ZKAMD_COOP_VERIFY", "0")
    d = plan(emu_lib, 16)
    assert d == want(LANES, 0, 1, TRI, 16, FOUR, 1, LANES18)
    assert changed(base, d) == {"decode", "prepare", "prep_b_points", "inputs", "pairing"}
    assert plan(emu_lib, 300) == want(LANES, 0, 1, TRI, 300, WINDOWS, 1, LANES18)
    assert plan(emu_lib, 2049) == want(LANES, 0, 1, TRI, 2049, WINDOWS, 1, LANES18)    # (what 2049 proofs run anyway)
    for on in ("", "1", "7"):   # unset or empty: the default
        monkeypatch.setenv("ZKAMD_COOP_VERIFY", on)
        assert plan(emu_lib, 16) == base


def test_coop_pairing_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 16)
    monkeypatch.setenv("ZKAMD_COOP_PAIRING", "0")
    d = plan(emu_lib, 16)
    # the eighteen lanes read B's lines from prep_b: the preparation on rows now writes them out
    assert d == want(ROWS, 0, 1, ROWS, 16, IN_ROWS, 1, LANES18)
    assert changed(base, d) == {"pairing", "prep_b_points"}
    assert plan(emu_lib, 2048) == want(ROWS, 0, 1, ROWS, 2048, WINDOWS, 1, LANES18)
    beyond = plan(emu_lib, 2049)
    for on in ("", "1"):
        monkeypatch.setenv("ZKAMD_COOP_PAIRING", on)
        assert plan(emu_lib, 16) == base
    assert plan(emu_lib, 2049) == beyond


def test_inputs_windows_variable(emu_lib, monkeypatch):
    base, small, bare = plan(emu_lib, 256), plan(emu_lib, 255), plan(emu_lib, 256, n_inputs=0)
    beyond = plan(emu_lib, 2049)
    monkeypatch.setenv("ZKAMD_INPUTS_WINDOWS", "0")
    d = plan(emu_lib, 256)
    assert d["inputs"] == SIXTEEN and changed(base, d) == {"inputs"}
    assert changed(beyond, plan(emu_lib, 2049)) == {"inputs"} and plan(emu_lib, 2049)["inputs"] == SIXTEEN
    assert plan(emu_lib, 255) == small and plan(emu_lib, 256, n_inputs=0) == bare
    monkeypatch.setenv("ZKAMD_INPUTS_WINDOWS", "")
    assert plan(emu_lib, 256) == base


def test_coop_inputs_max_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 16)
    monkeypatch.setenv("ZKAMD_COOP_INPUTS_MAX", "0")   # 0 is a value: the accumulator never on rows ...
    d = plan(emu_lib, 16)
    assert d["inputs"] == FOUR and changed(base, d) == {"inputs"}
    # ... and the decoders, the preparation and the pairing still on rows up to 2048 proofs
    assert plan(emu_lib, 1) == want(ROWS, 0, 1, ROWS, 0, FOUR, 1, P_ROWS)
    assert plan(emu_lib, 2048) == want(ROWS, 0, 1, ROWS, 0, WINDOWS, 1, P_ROWS)
    assert plan(emu_lib, 2049) == want(LANES, 0, 1, TRI, 2049, WINDOWS, 1, LANES18)
    monkeypatch.setenv("ZKAMD_COOP_INPUTS_MAX", "100")
    assert (plan(emu_lib, 100)["inputs"], plan(emu_lib, 101)["inputs"]) == (IN_ROWS, FOUR)
    # a bound above the pairing's keeps the head on rows with it: the eighteen lanes then read lines the rows wrote out
    monkeypatch.setenv("ZKAMD_COOP_INPUTS_MAX", "4096")
    assert plan(emu_lib, 3000) == want(ROWS, 0, 1, ROWS, 3000, IN_ROWS, 1, LANES18)
    assert plan(emu_lib, 4097) == want(LANES, 0, 1, TRI, 4097, WINDOWS, 1, LANES18)
    monkeypatch.setenv("ZKAMD_COOP_INPUTS_MAX", "")
    assert plan(emu_lib, 16) == base and plan(emu_lib, 65)["inputs"] == FOUR


def test_coop_pairing_max_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 8)
    monkeypatch.setenv("ZKAMD_COOP_PAIRING_MAX", "8")
    assert plan(emu_lib, 8) == base
    # up to the accumulator's 64 the head stays on rows, the pairing leaves them
    d = plan(emu_lib, 9)
    assert d == want(ROWS, 0, 1, ROWS, 9, IN_ROWS, 1, LANES18)
    assert plan(emu_lib, 64) == want(ROWS, 0, 1, ROWS, 64, IN_ROWS, 1, LANES18)
    assert plan(emu_lib, 65) == want(LANES, 0, 1, TRI, 65, FOUR, 1, LANES18)
    monkeypatch.setenv("ZKAMD_COOP_PAIRING_MAX", "8192")
    assert plan(emu_lib, 8192) == want(ROWS, 0, 1, ROWS, 0, WINDOWS, 1, P_ROWS)
    monkeypatch.setenv("ZKAMD_COOP_PAIRING_MAX", "0")
    assert plan(emu_lib, 1) == want(ROWS, 0, 1, ROWS, 1, IN_ROWS, 1, LANES18)
    monkeypatch.setenv("ZKAMD_COOP_PAIRING_MAX", "")
    assert stages(plan(emu_lib, 2048)) == (ROWS, ROWS, WINDOWS, P_ROWS) and stages(plan(emu_lib, 2049)) == (LANES, TRI, WINDOWS, LANES18)


def test_inputs_fine_min_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 100)
    assert base["inputs"] == FOUR
    monkeypatch.setenv("ZKAMD_INPUTS_FINE_MIN", "100")
    d = plan(emu_lib, 100)
    assert d["inputs"] == WINDOWS and changed(base, d) == {"inputs"}
    assert plan(emu_lib, 99)["inputs"] == FOUR and plan(emu_lib, 100, n_inputs=0)["inputs"] == SIXTEEN
    assert plan(emu_lib, 64)["inputs"] == IN_ROWS       # the rows come first
    monkeypatch.setenv("ZKAMD_INPUTS_FINE_MIN", "5000")
    assert plan(emu_lib, 4999)["inputs"] == FOUR and plan(emu_lib, 5000)["inputs"] == WINDOWS
    monkeypatch.setenv("ZKAMD_INPUTS_FINE_MIN", "")
    assert plan(emu_lib, 100) == base and plan(emu_lib, 256)["inputs"] == WINDOWS


def test_verify_rlc_min_variable_is_read_at_every_call(emu_lib, monkeypatch):
    base = plan(emu_lib, 100, form=AUTO)
    assert base["combined"] == 0
    monkeypatch.setenv("ZKAMD_VERIFY_RLC_MIN", "100")
    d = plan(emu_lib, 100, form=AUTO)
    assert d["combined"] == 1 and changed(base, d) == {"combined"}
    assert plan(emu_lib, 99, form=AUTO)["combined"] == 0
    assert plan(emu_lib, 100, form=PER_PROOF)["combined"] == 0 and plan(emu_lib, 8, form=COMBINED)["combined"] == 1
    monkeypatch.setenv("ZKAMD_VERIFY_RLC_MIN", "1")      # never below the 8 proofs the combined check needs
    assert [plan(emu_lib, n, form=AUTO)["combined"] for n in (7, 8)] == [0, 1]
    monkeypatch.setenv("ZKAMD_VERIFY_RLC_MIN", "")       # atoll: 0
    assert [plan(emu_lib, n, form=AUTO)["combined"] for n in (7, 8)] == [0, 1]
    monkeypatch.setenv("ZKAMD_VERIFY_RLC_MIN", "100000")
    assert plan(emu_lib, 8192, form=AUTO)["combined"] == 0 and plan(emu_lib, 8192, form=COMBINED)["combined"] == 1
    monkeypatch.delenv("ZKAMD_VERIFY_RLC_MIN")           # the same process, the next call: the default again
    assert [plan(emu_lib, n, form=AUTO)["combined"] for n in (4095, 4096)] == [0, 1]


# ------------------------------------------------------------------------------------------------------------------------
# (c) ZKAMD_VERIFY_WIDE=0: one thread per pair and per proof, no line preparation, B's r-torsion test inside its decoder
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", ["0", "", "abc"])      # off only when set and atoi() of it is 0: the empty string is off
def test_verify_wide_off(emu_lib, monkeypatch, value):
    base = plan(emu_lib, 2049)
    monkeypatch.setenv("ZKAMD_VERIFY_WIDE", value)
    for n, inputs in ((1, FOUR), (64, FOUR), (255, FOUR), (256, WINDOWS), (2049, WINDOWS)):   # no stage on rows either
        assert plan(emu_lib, n) == want(LANES, 1, 1, NONE, 0, inputs, 1, THREAD)
    assert plan(emu_lib, 256, n_inputs=0) == want(LANES, 1, 1, NONE, 0, SIXTEEN, 0, THREAD)
    assert changed(base, plan(emu_lib, 2049)) == {"b_torsion_in_decoder", "prepare", "prep_b_points", "pairing"}
    # the library's own proofs: no r-torsion test at all; with their coordinates no decoder
    assert plan(emu_lib, 1, own=True) == want(LANES, 0, 0, NONE, 0, FOUR, 1, THREAD)
    assert plan(emu_lib, 1, own=True, affine=True) == want(NONE, 0, 0, NONE, 0, FOUR, 1, THREAD)
    # the other switches of the rows have nothing left to switch
    wide_off = plan(emu_lib, 16)
    for name in ("ZKAMD_COOP_VERIFY", "ZKAMD_COOP_PAIRING"):
        monkeypatch.setenv(name, "0")
        assert plan(emu_lib, 16) == wide_off


@pytest.mark.parametrize("value", ["1", "2", "-1", "1x"])
def test_verify_wide_on(emu_lib, monkeypatch, value):
    base = [plan(emu_lib, n) for n in (1, 300, 2049)]
    monkeypatch.setenv("ZKAMD_VERIFY_WIDE", value)
    assert [plan(emu_lib, n) for n in (1, 300, 2049)] == base
