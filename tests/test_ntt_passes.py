"""The Fr transform pass by pass: every tile form of csrc/ntt.h k_ntt_pass that csrc/ntt_plan.h can plan, every option of
NttPlan::chain, every flag combination of zk_ntt_run_dev and every table of NttPlan::init, against Python integers and the C
restatement of bellman's fft (tests/ntt_cases.py).  The cases run on the x86 emulation build and - marked gpu - on
libzkamd_hooks.so; the plan pins use no GPU and run on the emulation build alone; of the transforms of 2^14 and more the
emulation build runs one 2^17 per tile form."""
import os

import pytest

import ntt_cases as nc
from ntt_cases import LATENCY, SMALL, MID, BIG, AUTO
from test_emu_pipeline import _host_alloc
from test_gpu_parity import _torch_alloc

# (form, k) of the pass-by-pass cases, each for DIF and DIT with the forward and the inverse twiddles
PASS_SHAPES = [(LATENCY, k) for k in (9, 10, 12, 13)] + [(SMALL, k) for k in (1, 2, 3, 7, 8, 9, 10, 13)]
PASS_CASES = [(f, k, dif, inv) for f, k in PASS_SHAPES for dif in (1, 0) for inv in (0, 1)]
OPTION_CASES = [(f, k, dif) for f, k in ((LATENCY, 10), (SMALL, 10), (MID, 17)) for dif in (1, 0)]
LARGE_CASES = [(f, k, b, dif, inv) for f, k, b in nc.LARGE for dif in (1, 0) for inv in (0, 1)]
_id = lambda c: "-".join([nc.FORM_NAMES[c[0]]] + [str(x) for x in c[1:]])


# ------------------------------------------------------------------------------------------------ a. the plan (no GPU)
def test_auto_form_thresholds(emu_lib):
    """latency while batch << k <= 2^17 for 2^9 .. 2^16, the 2^10-element tiles past it; mid from 2^17 on by default"""
    form = lambda k, batch, tiles=AUTO: nc.plan(emu_lib, k, batch, 1, tiles)[0]
    assert form(9, 256) == LATENCY and form(9, 257) == SMALL
    assert form(16, 2) == LATENCY and form(16, 3) == SMALL
    assert form(15, 4) == LATENCY and form(15, 5) == SMALL
    assert form(8, 1) == SMALL and form(16, 1) == LATENCY and form(15, 1024) == SMALL and form(16, 1024) == SMALL
    if "ZKAMD_NTT_TILES" not in os.environ:
        assert form(17, 1) == MID and form(20, 1) == MID and form(27, 1) == MID
    for tiles in (SMALL, MID, BIG):     # the tile choice given: from 2^17 on, whatever the batch; nothing below
        assert form(17, 1, 0x10 | tiles) == tiles and form(21, 1024, 0x10 | tiles) == tiles
        assert form(16, 3, 0x10 | tiles) == SMALL and form(16, 2, 0x10 | tiles) == LATENCY and form(3, 1, 0x10 | tiles) == SMALL


def test_pass_lists_of_the_product(emu_lib):
    """(t0, g, log_cw, dif, threads, grid_x, lds_bytes) per pass.  (15, 1024) and (16, 1024) are the benchmark's transforms."""
    P = lambda k, batch, dif, form: nc.plan(emu_lib, k, batch, dif, form)
    for dif in (1, 0):
        assert P(15, 1024, dif, AUTO) == (SMALL, [(0, 8, 2, dif, 256, 32, 32768), (8, 7, 3, dif, 256, 32, 32768)])
        assert P(16, 1024, dif, AUTO) == (SMALL, [(0, 8, 2, dif, 256, 64, 32768), (8, 8, 2, dif, 256, 64, 32768)])
        assert P(20, 1, dif, BIG) == (BIG, [(0, 10, 2, dif, 1024, 256, 131072), (10, 10, 2, dif, 1024, 256, 131072)])
        assert P(17, 1, dif, SMALL) == (SMALL, [(0, 6, 4, dif, 256, 128, 32768), (6, 6, 4, dif, 256, 128, 32768), (12, 5, 5, dif, 256, 128, 32768)])
        assert P(9, 256, dif, AUTO) == (LATENCY, [(0, 5, 3, dif, 128, 2, 8192), (5, 4, 4, dif, 128, 2, 8192)])
        assert P(16, 2, dif, AUTO) == (LATENCY, [(0, 8, 0, dif, 128, 256, 8192), (8, 8, 0, dif, 128, 256, 8192)])     # one-column tiles
        assert P(1, 1, dif, SMALL) == (SMALL, [(0, 1, 0, dif, 256, 1, 64)])
    # mid: the contiguous pass of 11 stages is the LAST of a DIF chain and the FIRST of a DIT chain
    assert P(20, 1, 1, MID) == (MID, [(0, 9, 2, 1, 512, 512, 65536), (9, 11, 0, 1, 512, 512, 65536)])
    assert P(20, 1, 0, MID) == (MID, [(0, 11, 0, 0, 512, 512, 65536), (11, 9, 2, 0, 512, 512, 65536)])
    assert P(21, 1, 1, MID) == (MID, [(0, 5, 6, 1, 512, 1024, 65536), (5, 5, 6, 1, 512, 1024, 65536), (10, 11, 0, 1, 512, 1024, 65536)])
    assert P(21, 1, 0, MID) == (MID, [(0, 11, 0, 0, 512, 1024, 65536), (11, 5, 6, 0, 512, 1024, 65536), (16, 5, 6, 0, 512, 1024, 65536)])
    assert P(11, 1, 1, MID) == (MID, [(0, 11, 0, 1, 512, 1, 65536)])
    assert P(10, 1, 1, MID) == nc.ZK_ERR_INVALID_ARGUMENT and P(10, 1, 0, MID) == nc.ZK_ERR_INVALID_ARGUMENT


def test_plan_invariants_every_form_and_size(emu_lib):
    assert nc.check_plan_invariants(emu_lib) == 2 * (27 + 27 + 17 + 27)


def test_reference_stages_against_the_oracles():
    """the stage functions composed are bellman's fft between the bit reversals (oracle/groth16.py through the C port), and the
    inverse twiddles give the transform of the sequence read backwards - the two facts the large cases rest on"""
    for k in (1, 4, 9):
        v = nc.unpack(nc.random_residues(k, 1 << k))
        for dif in (1, 0):
            for inverse in (0, 1):
                assert nc.stages(v, k, dif, inverse, 0, k) == nc.unpack(nc.c_fft(nc.pack(v), k, dif, inverse)), (k, dif, inverse)


# ------------------------------------------------------------------------------------------------ b. pass by pass
@pytest.mark.parametrize("case", PASS_CASES, ids=_id)
def test_passes_emulated(emu_lib, case):
    assert nc.check_passes(emu_lib, *case) >= 18


@pytest.mark.gpu
@pytest.mark.parametrize("case", PASS_CASES, ids=_id)
def test_passes_on_the_gpu(gpu_hooks_lib, case):
    assert nc.check_passes(gpu_hooks_lib, *case) >= 18


# ------------------------------------------------------------------------------------------------ c. chain options
@pytest.mark.parametrize("case", [c for c in OPTION_CASES if c[1] == 10], ids=_id)
def test_chain_options_emulated(emu_lib, case):
    nc.check_options(emu_lib, *case)


def test_size_one_chain_emulated(emu_lib):
    nc.check_size_one_chain(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", OPTION_CASES, ids=_id)
def test_chain_options_on_the_gpu(gpu_hooks_lib, case):
    nc.check_options(gpu_hooks_lib, *case)


@pytest.mark.gpu
def test_size_one_chain_on_the_gpu(gpu_hooks_lib):
    nc.check_size_one_chain(gpu_hooks_lib)


# ------------------------------------------------------------------------------------------------ d. tile forms from 2^14
@pytest.mark.parametrize("case", [(f, 17, 1, 1) for f in (SMALL, MID, BIG)], ids=_id)
def test_tile_forms_2p17_emulated(emu_lib, case):
    nc.check_large(emu_lib, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE_CASES, ids=_id)
def test_tile_forms_on_the_gpu(gpu_hooks_lib, case):
    nc.check_large(gpu_hooks_lib, *case)


# ------------------------------------------------------------------------------------------------ e. zk_ntt_run_dev
@pytest.mark.parametrize("k", [0, 1, 5, 9, 10, 12])
def test_run_dev_flag_combinations_emulated(emu_lib, k):
    assert nc.check_run_dev(emu_lib, k, _host_alloc(emu_lib)) == (12 if k else 16)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 5, 9, 10, 12])
def test_run_dev_flag_combinations_on_the_gpu(gpu_lib, k):
    assert nc.check_run_dev(gpu_lib, k, _torch_alloc()) == (12 if k else 16)


# ------------------------------------------------------------------------------------------------ f. the tables
@pytest.mark.parametrize("k", [0, 1, 2, 9])
def test_tables_emulated(emu_lib, k):
    nc.check_tables(emu_lib, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 9])
def test_tables_on_the_gpu(gpu_hooks_lib, k):
    nc.check_tables(gpu_hooks_lib, k)
