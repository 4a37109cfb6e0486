"""The plan of one chunk of the prover (csrc/prove_plan.h) pinned without a GPU, through the test hook zk_hook_prove_plan of
the emulation build: (a) the default forms on both sides of every threshold, (b) each of the eight environment variables
moves the fields it names and no other, (c) every section offset of the merged C job and of the witness vector.

Every form gives the same proof bytes (the parity suites hold them to that), so a threshold that moves by accident passes
every parity test and only changes what a call costs, and an offset that two users of the layout compute differently sends a
scalar to the wrong base: this file sees both.  The expected values are literals read off prove_chunk / ensure_maps /
k_build_scalars as they stood before the plan was split out of them, never the output of prove_plan.h."""
import ctypes as C

import pytest

# the order of the words zk_hook_prove_plan returns (csrc/zkamd.cpp)
PLAN = "fold_in_msm host_norm g2_lone split one_stream g1 map".split()
TUN = "batch_chunk host_chunk trace_host".split()
LAYOUT = ("n_in n_aux head ga gb2 gb1 fold derived w_one w_sum_a w_sum_b2 wstride aux rz r sz s rs in_tail sum_b1 sum_a "
          "cstride").split()
FIELDS = PLAN + TUN + LAYOUT
TUNABLES = ("ZKAMD_BATCH_CHUNK", "ZKAMD_HOST_CHUNK", "ZKAMD_FOLD_IN_MSM_MAX", "ZKAMD_G2_LONE_MAX", "ZKAMD_HOST_NORMALIZE_MAX",
            "ZKAMD_SPLIT_MIN", "ZKAMD_NO_OVERLAP", "ZKAMD_TRACE_HOST")
G1, G1_LONE, G1D, G1D_LONE = 0, 1, 2, 3       # the group of the C' jobs: the key's or the derived set's, of a batch or of a few proofs
MAP_C, MAP_CF, MAP_CD, MAP_CFD = 0, 1, 2, 3   # its map: key or derived (D) bases, without or with the fold (F)
# what the fold adds to a job over the key's bases / over the derived bases (whose inputs section moves behind it)
FOLD_FIELDS = {"fold_in_msm", "map", "fold", "sz", "s", "rs", "sum_b1", "sum_a", "cstride"}
# the shape of (c): 3 inputs, 5 aux variables, 6 live rows, a domain of 8; one group in A, two in B2, one in B1
SHAPE = dict(n_in=3, n_aux=5, n_rows=6, m=8, ga=1, gb2=2, gb1=1)


@pytest.fixture(autouse=True)
def _no_tunables(monkeypatch):
    for name in TUNABLES:   # (ZKAMD_SPLIT_MIN: the GPU suite's fixture sets it for the whole session)
        monkeypatch.delenv(name, raising=False)


def plan(lib, np, derived=False, n_in=3, n_aux=5, n_rows=6, m=8, ga=1, gb2=2, gb1=1):
    fn = lib.dll.zk_hook_prove_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                   C.POINTER(C.c_uint64), C.c_size_t]
    out = (C.c_uint64 * len(FIELDS))()
    lib.check(fn(np, n_in, n_aux, n_rows, m, ga, gb2, gb1, int(derived), out, len(out)))
    return dict(zip(FIELDS, out))


def forms(d):
    return tuple(d[k] for k in PLAN)


def changed(a, b):
    return {k for k in FIELDS if a[k] != b[k]}


# ------------------------------------------------------------------------------------------------------------------------
# (a) the defaults: the narrow G2 window up to 2 proofs, into_affine on the host up to 16, two G1 launch sets from 64, the fold
# inside the C multiexp up to 128; one stream never
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np, fold, host_norm, g2_lone, split", [
    (1, 1, 1, 1, 0), (2, 1, 1, 1, 0), (3, 1, 1, 0, 0), (16, 1, 1, 0, 0), (17, 1, 0, 0, 0), (63, 1, 0, 0, 0), (64, 1, 0, 0, 1),
    (128, 1, 0, 0, 1), (129, 0, 0, 0, 1), (1024, 0, 0, 0, 1)])
def test_default_forms_on_both_sides_of_every_threshold(emu_lib, np, fold, host_norm, g2_lone, split):
    assert forms(plan(emu_lib, np)) == (fold, host_norm, g2_lone, split, 0, G1 if split else G1_LONE, MAP_CF if fold else MAP_C)
    assert forms(plan(emu_lib, np, derived=True)) == (fold, host_norm, g2_lone, split, 0, G1D if split else G1D_LONE,
                                                      MAP_CFD if fold else MAP_CD)
    d = plan(emu_lib, np)
    assert (d["batch_chunk"], d["host_chunk"], d["trace_host"]) == (1024, 0, 0)
    assert d["fold"] == fold and plan(emu_lib, np, derived=True)["fold"] == fold


# ------------------------------------------------------------------------------------------------------------------------
# (b) the eight variables
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, field, unset", [("ZKAMD_BATCH_CHUNK", "batch_chunk", 1024), ("ZKAMD_HOST_CHUNK", "host_chunk", 0)])
def test_chunk_variables_are_ignored_unless_positive(emu_lib, monkeypatch, name, field, unset):
    base = plan(emu_lib, 100)
    assert base[field] == unset
    monkeypatch.setenv(name, "7")
    d = plan(emu_lib, 100)
    assert d[field] == 7 and changed(base, d) == {field}
    monkeypatch.setenv(name, "3000")
    assert plan(emu_lib, 100)[field] == 3000
    for ignored in ("0", "", "-3", "abc"):
        monkeypatch.setenv(name, ignored)
        assert plan(emu_lib, 100) == base
    monkeypatch.setenv(name, "12abc")   # atoi
    assert plan(emu_lib, 100)[field] == 12


def test_fold_in_msm_max_variable(emu_lib, monkeypatch):
    base, base_d, beyond = plan(emu_lib, 100), plan(emu_lib, 100, derived=True), plan(emu_lib, 129)
    assert (base["fold_in_msm"], base["map"], base_d["map"]) == (1, MAP_CF, MAP_CFD)
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "99")
    d, dd = plan(emu_lib, 100), plan(emu_lib, 100, derived=True)
    assert (d["fold_in_msm"], d["map"], dd["map"]) == (0, MAP_C, MAP_CD)
    assert changed(base, d) == FOLD_FIELDS and changed(base_d, dd) == FOLD_FIELDS | {"in_tail"}
    assert plan(emu_lib, 99)["fold_in_msm"] == 1 and plan(emu_lib, 129) == beyond
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")    # the chunk form of the fold for every chunk
    assert [plan(emu_lib, n)["fold_in_msm"] for n in (1, 128)] == [0, 0]
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "")     # atoll: 0
    assert [plan(emu_lib, n)["fold_in_msm"] for n in (1, 128)] == [0, 0]
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "5000")
    assert changed(beyond, plan(emu_lib, 129)) == FOLD_FIELDS and plan(emu_lib, 5000)["map"] == MAP_CF
    assert plan(emu_lib, 5001)["map"] == MAP_C
    monkeypatch.delenv("ZKAMD_FOLD_IN_MSM_MAX")         # the same process, the next chunk: the default again
    assert plan(emu_lib, 100) == base and plan(emu_lib, 129) == beyond


@pytest.mark.parametrize("name, field, last, np_inside, np_outside", [
    ("ZKAMD_G2_LONE_MAX", "g2_lone", 2, 8, 9), ("ZKAMD_HOST_NORMALIZE_MAX", "host_norm", 16, 40, 41)])
def test_g2_lone_max_and_host_normalize_max_are_read_at_every_chunk(emu_lib, monkeypatch, name, field, last, np_inside, np_outside):
    """(function-local statics until the plan was split out: the one intended difference)"""
    base = plan(emu_lib, np_inside)
    assert base[field] == 0 and [plan(emu_lib, n)[field] for n in (last, last + 1)] == [1, 0]
    monkeypatch.setenv(name, str(np_inside))
    d = plan(emu_lib, np_inside)
    assert d[field] == 1 and changed(base, d) == {field}
    assert plan(emu_lib, np_outside)[field] == 0
    for never in ("0", ""):   # atoll: 0
        monkeypatch.setenv(name, never)
        assert plan(emu_lib, 1)[field] == 0 and changed(plan(emu_lib, np_inside), base) == set()
    monkeypatch.delenv(name)
    assert [plan(emu_lib, n)[field] for n in (last, last + 1)] == [1, 0]


def test_split_min_variable(emu_lib, monkeypatch):
    base, base_d, many = plan(emu_lib, 2), plan(emu_lib, 2, derived=True), plan(emu_lib, 64)
    assert (base["split"], base["g1"], base_d["g1"]) == (0, G1_LONE, G1D_LONE)
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "2")
    d, dd = plan(emu_lib, 2), plan(emu_lib, 2, derived=True)
    assert (d["split"], d["g1"], dd["g1"]) == (1, G1, G1D)
    assert changed(base, d) == {"split", "g1"} and changed(base_d, dd) == {"split", "g1"}
    assert plan(emu_lib, 1)["split"] == 0 and plan(emu_lib, 64) == many
    for always in ("1", "0", ""):   # atoll: 0
        monkeypatch.setenv("ZKAMD_SPLIT_MIN", always)
        assert (plan(emu_lib, 1)["split"], plan(emu_lib, 1)["g1"]) == (1, G1)
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "100000")
    assert changed(many, plan(emu_lib, 64)) == {"split", "g1"} and plan(emu_lib, 1024)["g1"] == G1_LONE
    monkeypatch.delenv("ZKAMD_SPLIT_MIN")
    assert [plan(emu_lib, n)["split"] for n in (63, 64)] == [0, 1]


@pytest.mark.parametrize("name, field", [("ZKAMD_NO_OVERLAP", "one_stream"), ("ZKAMD_TRACE_HOST", "trace_host")])
def test_switches_by_presence_alone(emu_lib, monkeypatch, name, field):
    base = [plan(emu_lib, n) for n in (1, 100, 1024)]
    assert [d[field] for d in base] == [0, 0, 0]
    for value in ("1", "0", ""):
        monkeypatch.setenv(name, value)
        for n, b in zip((1, 100, 1024), base):
            d = plan(emu_lib, n)
            assert d[field] == 1 and changed(b, d) == {field}
    monkeypatch.delenv(name)
    assert [plan(emu_lib, n) for n in (1, 100, 1024)] == base


# ------------------------------------------------------------------------------------------------------------------------
# (c) the layout: 3 inputs, 5 aux variables (nv = 8), 6 live rows, a domain of 8, groups 1 / 2 / 1
#   witness vector  [ inputs 0 | aux 3 | 1 8 | r 9 | s 10 | sums of A 11 | sums of B2 12, 13 ]
#   C job           [ H block | aux | r z | r | (fold: s z | s | r s) | (derived: inputs) | r * sums of B1 | (fold: s * sums of A) ]
# np = 1: the fold inside the multiexp; np = 129: its own kernel
# ------------------------------------------------------------------------------------------------------------------------
WITNESS = dict(n_in=3, n_aux=5, ga=1, gb2=2, gb1=1, w_one=8, w_sum_a=11, w_sum_b2=12, wstride=14)
ABSENT = 0   # the offset of a section the form does not have


@pytest.mark.parametrize("derived, np, want", [
    (False, 129, dict(head=8, fold=0, derived=0, aux=8, rz=13, r=21, sz=ABSENT, s=ABSENT, rs=ABSENT, in_tail=ABSENT,
                      sum_b1=22, sum_a=ABSENT, cstride=23)),
    (False, 1, dict(head=8, fold=1, derived=0, aux=8, rz=13, r=21, sz=22, s=30, rs=31, in_tail=ABSENT,
                    sum_b1=32, sum_a=33, cstride=34)),
    (True, 129, dict(head=12, fold=0, derived=1, aux=12, rz=17, r=25, sz=ABSENT, s=ABSENT, rs=ABSENT, in_tail=26,
                     sum_b1=29, sum_a=ABSENT, cstride=30)),
    (True, 1, dict(head=12, fold=1, derived=1, aux=12, rz=17, r=25, sz=26, s=34, rs=35, in_tail=36,
                   sum_b1=39, sum_a=40, cstride=41)),
])
def test_layout_every_section_offset(emu_lib, derived, np, want):
    d = plan(emu_lib, np, derived=derived, **SHAPE)
    assert d["fold_in_msm"] == want["fold"]
    assert {k: d[k] for k in LAYOUT} == dict(WITNESS, **want)
    # the kernel this was read off took the sums of the groups from the END of the vector: with the fold its last ga slots
    # are s * sums of A and r * sums of B1 lie before them; without, r * sums of B1 are the last
    if want["fold"]:
        assert d["sum_a"] == d["cstride"] - SHAPE["ga"] and d["sum_b1"] == d["sum_a"] - SHAPE["gb1"]
    else:
        assert d["sum_b1"] == d["cstride"] - SHAPE["gb1"]


def test_layout_without_groups_and_with_wider_ones(emu_lib):
    """ZKAMD_MERGE_BASES=0 gives maps without groups: the vectors end behind s and behind r (fold: r s)"""
    none = dict(SHAPE, ga=0, gb2=0, gb1=0)
    d = plan(emu_lib, 129, **none)
    assert (d["wstride"], d["w_sum_a"], d["w_sum_b2"], d["sum_b1"], d["cstride"]) == (11, 11, 11, 22, 22)
    d = plan(emu_lib, 1, **none)
    assert (d["rs"], d["sum_b1"], d["sum_a"], d["cstride"]) == (31, 32, 32, 32)
    d = plan(emu_lib, 1, derived=True, **dict(SHAPE, ga=4, gb2=3, gb1=3))
    assert (d["w_sum_a"], d["w_sum_b2"], d["wstride"]) == (11, 15, 18)
    assert (d["in_tail"], d["sum_b1"], d["sum_a"], d["cstride"]) == (36, 39, 42, 46)
