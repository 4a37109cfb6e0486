"""The plan of a multiexp launch set (csrc/msm_plan.h) pinned without a GPU, through the test hook zk_hook_msm_plan of the
emulation build: (a) the launch sets of the product - literals printed by the parent commit's enqueue,
profiles/r09_msm_launch_plan.txt - (b) the flips at the documented thresholds (README.md's table of variables,
DESIGN.md 4.1), (c) each of the eight environment variables changes the field it names and nothing else.

A threshold that moves by accident still gives correct proofs (the bytes do not depend on the order of summation), so the
proof-byte suites cannot see it: this file does."""
import ctypes as C

import pytest

# the order of the words zk_hook_msm_plan returns (csrc/msm_g1.cpp), then n_jobs x pair_base and n_jobs x tbase
FIELDS = ("seg few coop_l1 coop_rb merge_inline heavy_cap light_cap use_light big_launch acc_asm red_asm L T nbits log2_2l "
          "s_stride nsplit lds_sort fine_log n_coarse coarse_wgs heavy_blocks medium_max max_n total total_tasks n_buckets n_class "
          "jobs_d cnt_off_toff ntasks_tbase hist heavy light tclass sorted tsums pairs red_r red_w red_t pin_jobs rank blockbase "
          "coarse redo result nj").split()
TUNABLES = ("ZKAMD_MSM_SEG", "ZKAMD_MSM_SEG_G2", "ZKAMD_FEW_JOBS", "ZKAMD_COOP_L1_MAX", "ZKAMD_ASM_MIN_PAIRS", "ZKAMD_NO_LDS_SORT",
            "ZKAMD_SORT_FINE_LOG", "ZKAMD_MERGE_SPLIT_MIN")
ZK_ERR_INVALID_ARGUMENT = 16   # include/zkamd.h


@pytest.fixture(autouse=True)
def _no_tunables(monkeypatch):
    for name in TUNABLES:
        monkeypatch.delenv(name, raising=False)


def plan(lib, group, c, sizes, vb_digit=0, asm=True, asm_reduce=None):
    """The plan of the launch set `sizes` (scalars per job) in a group of window c; asm: the build has the generated loops (the
    product: both, and level 1 for G1 only - msm_group.h asm_loop / asm_reduce).  A dict of FIELDS + pair_base + tbase."""
    fn = lib.dll.zk_hook_msm_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_size_t]
    nj = len(sizes)
    n = (C.c_uint32 * nj)(*sizes)
    out = (C.c_uint64 * (len(FIELDS) + 2 * nj))()
    if asm_reduce is None:
        asm_reduce = asm and group == 1
    lib.check(fn(int(group == 2), c, n, nj, vb_digit, int(asm), int(asm_reduce), out, len(out)))
    d = dict(zip(FIELDS, out[:len(FIELDS)]))
    assert d["nj"] == nj
    d["pair_base"] = list(out[len(FIELDS):len(FIELDS) + nj])
    d["tbase"] = list(out[len(FIELDS) + nj:])
    return d


def refusal(lib, *args, **kw):
    from zero_chain_amd._lib import ZkError
    with pytest.raises(ZkError) as e:
        plan(lib, *args, **kw)
    assert e.value.status == ZK_ERR_INVALID_ARGUMENT
    return str(e.value)


def parse_recorded(line):
    """One '[plan] ...' line of profiles/r09_msm_launch_plan.txt -> (group, c, sizes, vb_digit, expected fields, pair_base, tbase)"""
    head, fields, sizes_b, pb, tb = [s.strip() for s in line.split("|")]
    h = head.split()
    assert h[0] == "[plan]"
    kv = dict(x.split("=") for x in h[2:])
    sizes = []
    for run in kv["n"].split(","):
        n, k = run.split("x")
        sizes += [int(n)] * int(k)
    want = {k: int(v) for k, v in (x.split("=") for x in fields.split())}
    want.update({k: int(v) for k, v in (x.split("=") for x in sizes_b.split()[1:])})
    idx = lambda s: {int(x[1:x.index("]")]): int(x.split("=")[1]) for x in s.split()[1:]}
    return (2 if h[1] == "G2" else 1), int(kv["c"]), sizes, int(kv["vb_digit"]), want, idx(pb), idx(tb)


# ------------------------------------------------------------------------------------------------------------------------
# (b) the documented thresholds (README.md: the table of variables; the comments of csrc/msm_plan.h)
# ------------------------------------------------------------------------------------------------------------------------

def test_few_jobs_form_up_to_128_jobs_and_for_every_variable_base_set(emu_lib):
    assert plan(emu_lib, 1, 14, [1000] * 128)["few"] == 1
    assert plan(emu_lib, 1, 14, [1000] * 129)["few"] == 0
    assert plan(emu_lib, 2, 13, [1000] * 128)["few"] == 1
    assert plan(emu_lib, 2, 13, [1000] * 129)["few"] == 0
    for vb_digit in (1, 2, 17):
        assert plan(emu_lib, 1, 14, [1000] * 129, vb_digit=vb_digit)["few"] == 1
        assert plan(emu_lib, 2, 13, [1000] * 1024, vb_digit=vb_digit)["few"] == 1
    # what hangs on the form: the lists of the merge, the workspace of the bit planes, the blocks of the heavy list
    few, many = plan(emu_lib, 1, 14, [1000] * 128), plan(emu_lib, 1, 14, [1000] * 129)
    assert (few["use_light"], few["light"], many["use_light"]) == (0, 0, 1) and many["light"] == 4 * many["light_cap"]
    assert few["red_t"] > 0 and many["red_t"] == 0


def test_merge_and_level_1_on_rows_up_to_131072_buckets_g1_16384_g2(emu_lib):
    # nj nb at the bound exactly: eight digit positions of 16 384 buckets (G1), four of 4 096 (G2) ...
    assert plan(emu_lib, 1, 16, [1 << 17] * 8, vb_digit=1)["coop_l1"] == 1
    assert plan(emu_lib, 1, 16, [1 << 17] * 9, vb_digit=1)["coop_l1"] == 0
    assert plan(emu_lib, 2, 14, [1 << 17] * 4, vb_digit=1)["coop_l1"] == 1
    assert plan(emu_lib, 2, 14, [1 << 17] * 5, vb_digit=1)["coop_l1"] == 0
    # ... and one bucket beyond it (c = 2: one bucket per job)
    for group, bound in ((1, 131072), (2, 16384)):
        at, over = plan(emu_lib, group, 2, [1] * bound, vb_digit=1), plan(emu_lib, group, 2, [1] * (bound + 1), vb_digit=1)
        assert (at["n_buckets"], at["coop_l1"]) == (bound, 1)
        assert (over["n_buckets"], over["coop_l1"]) == (bound + 1, 0)
    # never for a chunk of proofs, and what hangs on it: nodes of LEVEL1_FAN = 4 buckets with one S each
    assert plan(emu_lib, 1, 14, [1000] * 129)["coop_l1"] == 0
    d = plan(emu_lib, 1, 16, [1 << 17] * 8, vb_digit=1)
    assert (d["L"], d["T"], d["s_stride"], d["merge_inline"]) == (4, 4096, 1, 8 * d["coop_rb"])


def test_assembly_loops_from_4_000_000_pairs_g1_1_000_000_g2(emu_lib):
    for group, bound in ((1, 4000000), (2, 1000000)):
        under, at = plan(emu_lib, group, 14, [bound - 1], vb_digit=1), plan(emu_lib, group, 14, [bound], vb_digit=1)
        assert (under["total"], under["big_launch"], under["acc_asm"], under["redo"]) == (bound - 1, 0, 0, 0)
        assert (at["total"], at["big_launch"], at["acc_asm"]) == (bound, 1, 1) and at["redo"] == 4 * at["total_tasks"]
        assert plan(emu_lib, group, 14, [bound], vb_digit=1, asm=False)["acc_asm"] == 0   # a build without the loops
    # level 1 in assembly: G1, many jobs (c = 14: 20 digits per scalar, 129 jobs of 200 000 scalars together) ...
    at = plan(emu_lib, 1, 14, [1550] * 128 + [1600])
    under = plan(emu_lib, 1, 14, [1550] * 128 + [1599])
    assert (at["total"], at["big_launch"], at["acc_asm"], at["red_asm"], at["L"], at["s_stride"]) == (4000000, 1, 1, 1, 32, 1)
    assert (under["total"], under["big_launch"], under["acc_asm"], under["red_asm"]) == (3999980, 0, 0, 0)
    # ... never for a few jobs, however large, never for G2, and not without the loop
    few = plan(emu_lib, 1, 14, [1 << 20] * 128)
    assert (few["few"], few["big_launch"], few["acc_asm"], few["red_asm"]) == (1, 1, 1, 0)
    assert plan(emu_lib, 2, 14, [1 << 20] * 129)["red_asm"] == 0
    assert plan(emu_lib, 1, 14, [1550] * 128 + [1600], asm_reduce=False)["red_asm"] == 0


def test_three_task_lengths_at_their_two_boundaries(emu_lib):
    # short tasks (32 points, G2: 16) below 4 000 000 pairs ...
    for group, short in ((1, 32), (2, 16)):
        assert plan(emu_lib, group, 14, [3999999], vb_digit=1)["seg"] == short
        assert plan(emu_lib, group, 14, [4000000], vb_digit=1)["seg"] == 64
        # ... 256 from 100 000 000 pairs in at least 64 jobs
        assert plan(emu_lib, group, 14, [1562500] * 63 + [1562499], vb_digit=1)["seg"] == 64
        assert plan(emu_lib, group, 14, [1562500] * 64, vb_digit=1)["seg"] == 256
        assert plan(emu_lib, group, 14, [1600000] * 63, vb_digit=1)["seg"] == 64
    # (the same through the digits of a table job: c = 14, 20 digits per scalar)
    assert plan(emu_lib, 1, 14, [199999])["seg"] == 32 and plan(emu_lib, 1, 14, [200000])["seg"] == 64
    d = plan(emu_lib, 1, 14, [200000])
    assert (d["n_class"], d["tclass"], d["hist"]) == (64, 256, (2 * 64 + 6) * 4)


def test_lds_sort_while_a_job_histogram_fits_64_kib_and_never_for_a_few_jobs(emu_lib):
    at, over = plan(emu_lib, 1, 16, [1000] * 129), plan(emu_lib, 1, 17, [1000] * 129)
    assert (at["cnt_off_toff"] // 129, at["lds_sort"]) == (65536, 1)
    assert (over["cnt_off_toff"] // 129, over["lds_sort"]) == (131072, 0)
    assert (at["fine_log"], at["n_coarse"], at["coarse_wgs"], at["rank"], at["blockbase"], at["coarse"]) == (0, 0, 0, 0, 0, 0)
    assert (over["fine_log"], over["n_coarse"], over["coarse_wgs"]) == (7, 256, 1)
    assert (over["rank"], over["blockbase"], over["coarse"]) == (8 * over["total"], 129 * 256 * 4, 4 * 129 * 256 * 4)
    assert plan(emu_lib, 1, 16, [1000] * 128)["lds_sort"] == 0


def test_refusals(emu_lib, monkeypatch):
    # 2^32 pairs
    assert refusal(emu_lib, 1, 14, [1 << 31, 1 << 31], vb_digit=1).endswith("too many (digit, point) pairs in one launch")
    assert plan(emu_lib, 1, 14, [1 << 31, (1 << 31) - (1 << 27)], vb_digit=1)["total"] == (1 << 32) - (1 << 27)
    # 2^32 tasks (every bucket may hold one)
    assert refusal(emu_lib, 1, 22, [1] * 4096).endswith("too many (digit, point) pairs in one launch")
    # 2^32 buckets: a set of that many buckets has more tasks than that, so the refusal above speaks first and
    # "too many buckets in one launch" stays behind it
    assert "too many" in refusal(emu_lib, 1, 22, [1] * 4097)
    # a sort whose fine bins do not fit (more than MSM_FINE_MAX = 2048 buckets per bin)
    monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", "12")
    assert refusal(emu_lib, 1, 16, [1000]).endswith("ZKAMD_SORT_FINE_LOG out of range")
    assert plan(emu_lib, 1, 16, [1000] * 129)["lds_sort"] == 1   # (the LDS sort has no fine bins)


# ------------------------------------------------------------------------------------------------------------------------
# (c) the eight variables
# ------------------------------------------------------------------------------------------------------------------------
PRIMARY = ("seg", "few", "coop_l1", "big_launch", "lds_sort", "medium_max")   # what the variables name (+ fine_log, below)


def changed(a, b, keys=PRIMARY):
    return {k for k in keys if a[k] != b[k]}


def test_msm_seg_variables(emu_lib, monkeypatch):
    # (129 jobs at c = 17: neither the form nor the sort hangs on what the variable changes)
    base1, base2 = plan(emu_lib, 1, 17, [1000] * 129), plan(emu_lib, 2, 17, [1000] * 129)
    assert (base1["seg"], base2["seg"]) == (32, 16)
    monkeypatch.setenv("ZKAMD_MSM_SEG", "100")
    g1, g2 = plan(emu_lib, 1, 17, [1000] * 129), plan(emu_lib, 2, 17, [1000] * 129)
    assert (g1["seg"], g2["seg"]) == (100, 100)            # G2 falls back to the common variable
    assert changed(base1, g1) == {"seg"} and changed(base2, g2) == {"seg"}
    assert (g1["fine_log"], g1["n_class"]) == (base1["fine_log"], 129 * 100)
    monkeypatch.setenv("ZKAMD_MSM_SEG_G2", "48")
    assert (plan(emu_lib, 1, 17, [1000] * 129)["seg"], plan(emu_lib, 2, 17, [1000] * 129)["seg"]) == (100, 48)
    monkeypatch.setenv("ZKAMD_MSM_SEG_G2", "999")            # set: it is the one G2 reads - and out of range: ignored
    assert (plan(emu_lib, 1, 17, [1000] * 129)["seg"], plan(emu_lib, 2, 17, [1000] * 129)["seg"]) == (100, 16)
    monkeypatch.delenv("ZKAMD_MSM_SEG")
    monkeypatch.setenv("ZKAMD_MSM_SEG_G2", "48")
    assert (plan(emu_lib, 1, 17, [1000] * 129)["seg"], plan(emu_lib, 2, 17, [1000] * 129)["seg"]) == (32, 48)
    monkeypatch.delenv("ZKAMD_MSM_SEG_G2")
    for ok in ("1", "256"):
        monkeypatch.setenv("ZKAMD_MSM_SEG", ok)
        assert plan(emu_lib, 1, 17, [1000] * 129)["seg"] == int(ok)
    for ignored in ("0", "257", "-3", "abc", ""):
        monkeypatch.setenv("ZKAMD_MSM_SEG", ignored)
        assert plan(emu_lib, 1, 17, [1000] * 129) == base1


def test_few_jobs_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 17, [1000] * 8)
    assert base["few"] == 1 and base["coop_l1"] == 0
    monkeypatch.setenv("ZKAMD_FEW_JOBS", "1")
    assert changed(base, plan(emu_lib, 1, 17, [1000] * 8)) == {"few"}
    assert plan(emu_lib, 1, 17, [1000] * 1)["few"] == 1
    assert plan(emu_lib, 1, 17, [1000] * 8, vb_digit=3)["few"] == 1    # a variable-base set whatever the variable says
    monkeypatch.setenv("ZKAMD_FEW_JOBS", "2000")
    assert plan(emu_lib, 1, 17, [1000] * 2000)["few"] == 1 and plan(emu_lib, 1, 17, [1000] * 2001)["few"] == 0
    for ignored in ("0", "-5", "abc"):
        monkeypatch.setenv("ZKAMD_FEW_JOBS", ignored)
        assert plan(emu_lib, 1, 17, [1000] * 8) == base
        assert plan(emu_lib, 1, 17, [1000] * 129)["few"] == 0


def test_coop_l1_max_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 14, [20000, 90000])
    assert base["coop_l1"] == 1
    monkeypatch.setenv("ZKAMD_COOP_L1_MAX", "0")      # 0 is a value: never on rows
    assert changed(base, plan(emu_lib, 1, 14, [20000, 90000])) == {"coop_l1"}
    monkeypatch.setenv("ZKAMD_COOP_L1_MAX", "8192")
    assert plan(emu_lib, 1, 14, [20000, 90000])["coop_l1"] == 1 and plan(emu_lib, 1, 14, [20000, 90000, 1])["coop_l1"] == 0
    assert plan(emu_lib, 2, 14, [20000, 90000])["coop_l1"] == 1       # one bound for both groups when it is set
    monkeypatch.setenv("ZKAMD_COOP_L1_MAX", "1000000")
    assert plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1)["coop_l1"] == 1
    assert plan(emu_lib, 1, 14, [1000] * 129)["coop_l1"] == 0          # a chunk of proofs stays on lanes


def test_asm_min_pairs_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 14, [1000] * 129)
    assert (base["big_launch"], base["acc_asm"], base["red_asm"], base["redo"]) == (0, 0, 0, 0)
    monkeypatch.setenv("ZKAMD_ASM_MIN_PAIRS", "0")    # 0 is a value: every launch, however small
    d = plan(emu_lib, 1, 14, [1000] * 129)
    assert changed(base, d) == {"big_launch"} and (d["acc_asm"], d["red_asm"]) == (1, 1)
    assert plan(emu_lib, 1, 14, [0])["big_launch"] == 1
    assert plan(emu_lib, 1, 14, [1000] * 129, asm=False)["acc_asm"] == 0
    monkeypatch.setenv("ZKAMD_ASM_MIN_PAIRS", "2580001")
    assert plan(emu_lib, 1, 14, [1000] * 129)["big_launch"] == 0
    monkeypatch.setenv("ZKAMD_ASM_MIN_PAIRS", "2580000")
    assert plan(emu_lib, 1, 14, [1000] * 129)["big_launch"] == 1 and plan(emu_lib, 2, 14, [1000] * 129)["big_launch"] == 1


def test_no_lds_sort_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 14, [1000] * 129)
    assert base["lds_sort"] == 1
    monkeypatch.setenv("ZKAMD_NO_LDS_SORT", "1")
    d = plan(emu_lib, 1, 14, [1000] * 129)
    assert changed(base, d) == {"lds_sort"} and (d["fine_log"], d["n_coarse"]) == (7, 32)
    few = plan(emu_lib, 1, 14, [1000] * 8)
    monkeypatch.delenv("ZKAMD_NO_LDS_SORT")
    assert plan(emu_lib, 1, 14, [1000] * 8) == few    # the few-jobs form has no LDS sort to lose


def test_sort_fine_log_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 16, [5000] * 3)
    assert (base["fine_log"], base["n_coarse"], base["coarse_wgs"]) == (7, 128, 5)
    monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", "9")
    d = plan(emu_lib, 1, 16, [5000] * 3)
    assert changed(base, d) == set() and (d["fine_log"], d["n_coarse"]) == (9, 32)
    assert {k for k in d if d[k] != base[k]} == {"fine_log", "n_coarse", "blockbase", "coarse"}
    # raised until a job has at most MSM_COARSE_MAX = 1024 bins, lowered to the c - 2 bits a bucket index has
    monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", "1")
    assert plan(emu_lib, 1, 16, [5000] * 3)["fine_log"] == 4
    monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", "30")
    d = plan(emu_lib, 1, 12, [5000] * 3)
    assert (d["fine_log"], d["n_coarse"]) == (10, 1)
    monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", "11")
    assert plan(emu_lib, 1, 16, [5000] * 3)["fine_log"] == 11
    # more than MSM_FINE_MAX = 2048 buckets per bin: refused
    for bad in ("12", "30", "-1"):
        monkeypatch.setenv("ZKAMD_SORT_FINE_LOG", bad)
        assert refusal(emu_lib, 1, 16, [5000] * 3).endswith("ZKAMD_SORT_FINE_LOG out of range")


def test_merge_split_min_variable(emu_lib, monkeypatch):
    base = plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1)
    assert base["medium_max"] == 64                     # default 256: the eight-lane merge takes the buckets up to 64 partials
    monkeypatch.setenv("ZKAMD_MERGE_SPLIT_MIN", "32")
    d = plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1)
    assert d["medium_max"] == 32 and {k for k in d if d[k] != base[k]} == {"medium_max"}
    monkeypatch.setenv("ZKAMD_MERGE_SPLIT_MIN", "16")   # (what the suites set)
    assert plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1)["medium_max"] == 16
    monkeypatch.setenv("ZKAMD_MERGE_SPLIT_MIN", "1")    # never below the sixteen workgroups of the split form
    assert plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1)["medium_max"] == 16
    monkeypatch.setenv("ZKAMD_MERGE_SPLIT_MIN", "1000")
    assert plan(emu_lib, 1, 16, [1 << 20] * 17, vb_digit=1) == base


# ------------------------------------------------------------------------------------------------------------------------
# (a) the launch sets of the product, under the flags of the product build (both assembly loops, level 1 for G1).  The lines
# are those of profiles/r09_msm_launch_plan.txt, section (a): the locals of the PARENT commit's enqueue, printed by a
# throwaway patch of it - never the output of msm_plan.h.  (No MI355X was available when they were taken: the parent's
# enqueue was called on the CPU with the job lists prove_chunk / msm_run_dev build for these workloads, see the profile.
# To be replaced by the lines of a run on the device; they should not differ.)
# ------------------------------------------------------------------------------------------------------------------------
RECORDED = (
    # 1024-proof chunk
    "[plan] G1 c=16 nb=16384 maxd=17 nj=1024 vb_digit=0 to_host=0 n=72702x1024 | seg=256 few=0 coop_l1=0 coop_rb=1 merge_inline=8 heavy_cap=617968 light_cap=4943737 use_light=1 big_launch=1 acc_asm=1 red_asm=1 L=32 T=512 nbits=9 log2_2l=6 s_stride=1 nsplit=4 lds_sort=1 fine_log=0 n_coarse=0 coarse_wgs=0 heavy_blocks=4096 medium_max=64 max_n=72702 total=1265596416 total_tasks=21721088 n_buckets=16777216 n_class=262144 | bytes: jobs_d=40960 cnt_off_toff=67108864 ntasks_tbase=4096 hist=2097176 heavy=2471872 light=19774948 tclass=1048576 sorted=347537408 tsums=4865523712 pairs=5062385664 red_r=117440512 red_w=117669888 red_t=0 pin_jobs=45056 rank=0 blockbase=0 coarse=0 redo=86884352 result=196608 | pair_base: [0]=0 [1]=1235934 [1023]=1264360482 | tbase: [0]=0 [1]=21212 [1023]=21699876",
    "[plan] G1 c=14 nb=4096 maxd=20 nj=1024 vb_digit=0 to_host=0 n=19981x1024 | seg=256 few=0 coop_l1=0 coop_rb=1 merge_inline=8 heavy_cap=199811 light_cap=1598481 use_light=1 big_launch=1 acc_asm=1 red_asm=1 L=32 T=128 nbits=7 log2_2l=6 s_stride=1 nsplit=1 lds_sort=1 fine_log=0 n_coarse=0 coarse_wgs=0 heavy_blocks=4096 medium_max=64 max_n=19981 total=409210880 total_tasks=5793792 n_buckets=4194304 n_class=262144 | bytes: jobs_d=40960 cnt_off_toff=16777216 ntasks_tbase=4096 hist=2097176 heavy=799244 light=6393924 tclass=1048576 sorted=92700672 tsums=1297809408 pairs=1636843520 red_r=29360128 red_w=29589504 red_t=0 pin_jobs=45056 rank=0 blockbase=0 coarse=0 redo=23175168 result=196608 | pair_base: [0]=0 [1]=399620 [1023]=408811260 | tbase: [0]=0 [1]=5658 [1023]=5788134",
    "[plan] G2 c=13 nb=2048 maxd=21 nj=1024 vb_digit=0 to_host=0 n=19981x1024 | seg=256 few=0 coop_l1=0 coop_rb=1 merge_inline=8 heavy_cap=209801 light_cap=1678405 use_light=1 big_launch=1 acc_asm=1 red_asm=0 L=16 T=128 nbits=7 log2_2l=5 s_stride=16 nsplit=1 lds_sort=1 fine_log=0 n_coarse=0 coarse_wgs=0 heavy_blocks=4096 medium_max=64 max_n=19981 total=429671424 total_tasks=3776512 n_buckets=2097152 n_class=262144 | bytes: jobs_d=40960 cnt_off_toff=8388608 ntasks_tbase=4096 hist=2097176 heavy=839204 light=6713620 tclass=1048576 sorted=60424192 tsums=1691877376 pairs=1718685696 red_r=939524096 red_w=59179008 red_t=0 pin_jobs=45056 rank=0 blockbase=0 coarse=0 redo=15106048 result=393216 | pair_base: [0]=0 [1]=419601 [1023]=429251823 | tbase: [0]=0 [1]=3688 [1023]=3772824",
    # one proof alone
    "[plan] G1 c=15 nb=8192 maxd=18 nj=2 vb_digit=0 to_host=0 n=92682x1,19981x1 | seg=32 few=1 coop_l1=1 coop_rb=1 merge_inline=8 heavy_cap=7922 light_cap=63373 use_light=0 big_launch=0 acc_asm=0 red_asm=0 L=4 T=2048 nbits=11 log2_2l=3 s_stride=1 nsplit=16 lds_sort=0 fine_log=7 n_coarse=64 coarse_wgs=91 heavy_blocks=512 medium_max=64 max_n=92682 total=2027934 total_tasks=79758 n_buckets=16384 n_class=64 | bytes: jobs_d=80 cnt_off_toff=65536 ntasks_tbase=8 hist=536 heavy=31688 light=0 tclass=256 sorted=1276128 tsums=17865792 pairs=8111736 red_r=917504 red_w=917952 red_t=91392 pin_jobs=88 rank=16223472 blockbase=46592 coarse=2048 redo=0 result=384 | pair_base: [0]=0 [1]=1668276 | tbase: [0]=0 [1]=60326",
    "[plan] G2 c=10 nb=256 maxd=27 nj=1 vb_digit=0 to_host=0 n=19981x1 | seg=16 few=1 coop_l1=1 coop_rb=16 merge_inline=128 heavy_cap=264 light_cap=33718 use_light=0 big_launch=0 acc_asm=0 red_asm=0 L=4 T=64 nbits=6 log2_2l=3 s_stride=1 nsplit=1 lds_sort=0 fine_log=7 n_coarse=2 coarse_wgs=20 heavy_blocks=264 medium_max=64 max_n=19981 total=539487 total_tasks=33974 n_buckets=256 n_class=16 | bytes: jobs_d=40 cnt_off_toff=1024 ntasks_tbase=4 hist=152 heavy=1056 light=0 tclass=64 sorted=543584 tsums=15220352 pairs=2157948 red_r=28672 red_w=29120 red_t=3136 pin_jobs=44 rank=4315896 blockbase=160 coarse=32 redo=0 result=384 | pair_base: [0]=0 | tbase: [0]=0",
    # 8 proofs
    "[plan] G1 c=15 nb=8192 maxd=18 nj=16 vb_digit=0 to_host=0 n=92682x8,19981x8 | seg=64 few=1 coop_l1=1 coop_rb=1 merge_inline=8 heavy_cap=31687 light_cap=253492 use_light=0 big_launch=1 acc_asm=1 red_asm=0 L=4 T=2048 nbits=11 log2_2l=3 s_stride=1 nsplit=16 lds_sort=0 fine_log=7 n_coarse=64 coarse_wgs=91 heavy_blocks=512 medium_max=64 max_n=92682 total=16223472 total_tasks=384568 n_buckets=131072 n_class=1024 | bytes: jobs_d=640 cnt_off_toff=524288 ntasks_tbase=64 hist=8216 heavy=126748 light=0 tclass=4096 sorted=6153088 tsums=86143232 pairs=64893888 red_r=7340032 red_w=7343616 red_t=731136 pin_jobs=704 rank=129787776 blockbase=372736 coarse=16384 redo=1538272 result=3072 | pair_base: [0]=0 [1]=1668276 [2]=3336552 [3]=5004828 [4]=6673104 [5]=8341380 [6]=10009656 [7]=11677932 [8]=13346208 [9]=13705866 [10]=14065524 [11]=14425182 [12]=14784840 [13]=15144498 [14]=15504156 [15]=15863814 | tbase: [0]=0 [1]=34259 [2]=68518 [3]=102777 [4]=137036 [5]=171295 [6]=205554 [7]=239813 [8]=274072 [9]=287884 [10]=301696 [11]=315508 [12]=329320 [13]=343132 [14]=356944 [15]=370756",
    "[plan] G2 c=13 nb=2048 maxd=21 nj=8 vb_digit=0 to_host=0 n=19981x8 | seg=16 few=1 coop_l1=1 coop_rb=1 merge_inline=8 heavy_cap=26226 light_cap=209801 use_light=0 big_launch=1 acc_asm=1 red_asm=0 L=4 T=512 nbits=9 log2_2l=3 s_stride=1 nsplit=4 lds_sort=0 fine_log=7 n_coarse=16 coarse_wgs=20 heavy_blocks=512 medium_max=64 max_n=19981 total=3356808 total_tasks=226192 n_buckets=16384 n_class=128 | bytes: jobs_d=320 cnt_off_toff=65536 ntasks_tbase=32 hist=1048 heavy=104904 light=0 tclass=512 sorted=3619072 tsums=101334016 pairs=13427232 red_r=1835008 red_w=1838592 red_t=179200 pin_jobs=352 rank=26854464 blockbase=10240 coarse=2048 redo=904768 result=3072 | pair_base: [0]=0 [1]=419601 [2]=839202 [3]=1258803 [4]=1678404 [5]=2098005 [6]=2517606 [7]=2937207 | tbase: [0]=0 [1]=28274 [2]=56548 [3]=84822 [4]=113096 [5]=141370 [6]=169644 [7]=197918",
    # 2^20 G1 vb w=15, 2^17 G2 vb w=12, 2^17 G1 vb w=13
    "[plan] G1 c=16 nb=16384 maxd=1 nj=17 vb_digit=1 to_host=0 n=1048576x17 | seg=64 few=1 coop_l1=0 coop_rb=1 merge_inline=8 heavy_cap=34817 light_cap=278529 use_light=0 big_launch=1 acc_asm=1 red_asm=0 L=8 T=2048 nbits=11 log2_2l=4 s_stride=8 nsplit=16 lds_sort=0 fine_log=7 n_coarse=128 coarse_wgs=1024 heavy_blocks=512 medium_max=64 max_n=1048576 total=17825792 total_tasks=557073 n_buckets=278528 n_class=1088 | bytes: jobs_d=680 cnt_off_toff=1114112 ntasks_tbase=68 hist=8728 heavy=139268 light=0 tclass=4352 sorted=8913168 tsums=124784352 pairs=71303168 red_r=62390272 red_w=7802592 red_t=776832 pin_jobs=748 rank=142606336 blockbase=8912896 coarse=34816 redo=2228292 result=3264 | pair_base: [0]=0 [1]=1048576 [2]=2097152 [3]=3145728 [4]=4194304 [5]=5242880 [6]=6291456 [7]=7340032 [8]=8388608 [9]=9437184 [10]=10485760 [11]=11534336 [12]=12582912 [13]=13631488 [14]=14680064 [15]=15728640 [16]=16777216 | tbase: [0]=0 [1]=32769 [2]=65538 [3]=98307 [4]=131076 [5]=163845 [6]=196614 [7]=229383 [8]=262152 [9]=294921 [10]=327690 [11]=360459 [12]=393228 [13]=425997 [14]=458766 [15]=491535 [16]=524304",
    "[plan] G2 c=13 nb=2048 maxd=1 nj=22 vb_digit=1 to_host=0 n=131072x22 | seg=16 few=1 coop_l1=0 coop_rb=1 merge_inline=8 heavy_cap=22529 light_cap=180225 use_light=0 big_launch=1 acc_asm=1 red_asm=0 L=4 T=512 nbits=9 log2_2l=3 s_stride=4 nsplit=4 lds_sort=0 fine_log=7 n_coarse=16 coarse_wgs=128 heavy_blocks=512 medium_max=64 max_n=131072 total=2883584 total_tasks=225302 n_buckets=45056 n_class=352 | bytes: jobs_d=880 cnt_off_toff=180224 ntasks_tbase=88 hist=2840 heavy=90116 light=0 tclass=1408 sorted=3604832 tsums=100935296 pairs=11534336 red_r=20185088 red_w=5056128 red_t=492800 pin_jobs=968 rank=23068672 blockbase=180224 coarse=5632 redo=901208 result=8448 | pair_base: [0]=0 [1]=131072 [2]=262144 [3]=393216 [4]=524288 [5]=655360 [6]=786432 [7]=917504 [8]=1048576 [9]=1179648 [10]=1310720 [11]=1441792 [12]=1572864 [13]=1703936 [14]=1835008 [15]=1966080 [16]=2097152 [17]=2228224 [18]=2359296 [19]=2490368 [20]=2621440 [21]=2752512 | tbase: [0]=0 [1]=10241 [2]=20482 [3]=30723 [4]=40964 [5]=51205 [6]=61446 [7]=71687 [8]=81928 [9]=92169 [10]=102410 [11]=112651 [12]=122892 [13]=133133 [14]=143374 [15]=153615 [16]=163856 [17]=174097 [18]=184338 [19]=194579 [20]=204820 [21]=215061",
    "[plan] G1 c=14 nb=4096 maxd=1 nj=20 vb_digit=1 to_host=0 n=131072x20 | seg=32 few=1 coop_l1=1 coop_rb=1 merge_inline=8 heavy_cap=10241 light_cap=81921 use_light=0 big_launch=0 acc_asm=0 red_asm=0 L=4 T=1024 nbits=10 log2_2l=3 s_stride=1 nsplit=8 lds_sort=0 fine_log=7 n_coarse=32 coarse_wgs=128 heavy_blocks=512 medium_max=64 max_n=131072 total=2621440 total_tasks=163860 n_buckets=81920 n_class=640 | bytes: jobs_d=800 cnt_off_toff=327680 ntasks_tbase=80 hist=5144 heavy=40964 light=0 tclass=2560 sorted=2621760 tsums=36704640 pairs=10485760 red_r=4587520 red_w=4592000 red_t=443520 pin_jobs=880 rank=20971520 blockbase=327680 coarse=10240 redo=0 result=3840 | pair_base: [0]=0 [1]=131072 [2]=262144 [3]=393216 [4]=524288 [5]=655360 [6]=786432 [7]=917504 [8]=1048576 [9]=1179648 [10]=1310720 [11]=1441792 [12]=1572864 [13]=1703936 [14]=1835008 [15]=1966080 [16]=2097152 [17]=2228224 [18]=2359296 [19]=2490368 | tbase: [0]=0 [1]=8193 [2]=16386 [3]=24579 [4]=32772 [5]=40965 [6]=49158 [7]=57351 [8]=65544 [9]=73737 [10]=81930 [11]=90123 [12]=98316 [13]=106509 [14]=114702 [15]=122895 [16]=131088 [17]=139281 [18]=147474 [19]=155667",
)


def _id(line):
    h = line.split("|")[0].split()
    kv = dict(x.split("=") for x in h[2:])
    return "%s-c%s-%s%s" % (h[1], kv["c"], kv["n"].replace(",", "+"), "-vb" if kv["vb_digit"] != "0" else "")


@pytest.mark.parametrize("line", RECORDED, ids=[_id(l) for l in RECORDED])
def test_recorded_plan_of_a_product_launch_set(emu_lib, line):
    group, c, sizes, vb_digit, want, pair_base, tbase = parse_recorded(line)
    got = plan(emu_lib, group, c, sizes, vb_digit=vb_digit, asm=True)
    assert set(want) | {"nj"} == set(FIELDS)                      # every field of the plan is pinned
    assert {k: got[k] for k in want} == want
    assert pair_base and {k: got["pair_base"][k] for k in pair_base} == pair_base
    assert tbase and {k: got["tbase"][k] for k in tbase} == tbase
    # (the recorded lines list the first two jobs and the last one of a long set: all jobs of a run are equally long,
    #  so are the steps between them)
    for name in ("pair_base", "tbase"):
        steps = {(sizes[k], got[name][k + 1] - got[name][k]) for k in range(len(sizes) - 1)}
        assert len(steps) == len(set(sizes[:-1]))
