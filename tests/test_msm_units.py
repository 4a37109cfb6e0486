"""The multiexp's kernels by translation unit, without a GPU: csrc/msm.h is cut into headers by pass, a unit includes the
passes it launches, and where two units need one kernel a host function of msm_g1.cpp / msm_g2.cpp stands between them
(msm_group.h).  So every MSM kernel lies in exactly one code object of the library (tools/kernel_resources.py reads them), and
an edit to a sort kernel rebuilds the two units that include it (build._deps), not seven."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zero-chain_amd", "csrc")

# ntt.h's non-template kernels, compiled by the three units that include it: what is left of the copies, and may only shrink
NTT_SHARED = {"k_ntt_pass", "k_h_pointwise", "k_h_live_rows", "k_fr_scale", "k_fr_bitrev", "k_fr_pow_table", "k_fr_convert",
              "k_fr_first_noncanonical", "k_r1cs_eval", "k_build_scalars"}
SORT_KERNELS = ("k_msm_sort_lds", "k_msm_coarse_count", "k_msm_coarse_scan", "k_msm_coarse_scatter", "k_msm_fine_sort",
                "k_msm_task_offsets", "k_msm_task_hist", "k_msm_task_base", "k_msm_task_place")


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _plain(mangled):
    """k_name of _ZN5zkdevL<len>k_name...: the length prefix says where the name ends"""
    i = mangled.index("k_")
    j = i
    while mangled[j - 1].isdigit():
        j -= 1
    return mangled[i:i + int(mangled[j:i])]


def test_every_msm_kernel_lies_in_one_code_object():
    from zero_chain_amd import _lib
    objects = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources_per_object(_lib.LIB_PATH)
    assert len(objects) > 1
    holders = {}
    for k, obj in enumerate(objects):
        for name in obj:
            holders.setdefault(name, []).append(k)
    shared = {_plain(name) for name, ks in holders.items() if len(ks) > 1}
    assert shared <= NTT_SHARED, sorted(shared - NTT_SHARED)
    # the two group units, named by a kernel only they hold
    (g1,) = [k for k, obj in enumerate(objects) if any("k_msm_reduce1_redo" in n for n in obj)]
    (g2,) = [k for k, obj in enumerate(objects) if any("k_msm_accumulate_g2asm" in n for n in obj)]
    assert g1 != g2
    for name, ks in holders.items():
        if "g1asm" in name:
            assert ks == [g1], name
        if "g2asm" in name:
            assert ks == [g2], name
    # the sort and the task order do not depend on the group: msm_g1.cpp launches them for both
    for kernel in SORT_KERNELS:
        assert [ks for name, ks in holders.items() if _plain(name) == kernel] == [[g1]], kernel
    # two workgroups of the LDS sort per CU (msm_sort.h): 64 registers at the most, nothing in scratch memory
    (r,) = [r for name, r in objects[g1].items() if _plain(name) == "k_msm_sort_lds"]
    assert r["vgpr"] <= 64 and r["scratch"] == 0, r


def test_units_include_the_passes_they_launch():
    build = _load("zk_build", "zero-chain_amd", "build.py")
    deps = lambda unit: {os.path.basename(d) for d in build._deps(os.path.join(CSRC, unit))}
    generated = {"madd_asm.h", "red_asm.h"}
    passes = {"msm_sort.h", "msm_accumulate.h", "msm_asm_g1.h", "msm_asm_g2.h", "msm_reduce.h"}
    for unit in ("verify.cpp", "setup.cpp", "witness.cpp", "wallet.cpp", "zkamd.cpp"):
        d = deps(unit)
        assert not d & (generated | passes | {"msm.h", "msm_group_impl.h"}), (unit, sorted(d & (generated | passes)))
    g1, g2 = deps("msm_g1.cpp"), deps("msm_g2.cpp")
    assert generated | passes - {"msm_asm_g2.h"} <= g1 and "msm_asm_g2.h" not in g1
    assert {"madd_asm.h", "msm_accumulate.h", "msm_asm_g2.h", "msm_reduce.h"} <= g2
    assert not g2 & {"red_asm.h", "msm_sort.h", "msm_recode.h", "msm_asm_g1.h"}
    # an edit to a sort kernel rebuilds msm_g1.cpp and nothing else of the shipped library; the recoding, also the hooks' unit
    users = lambda header: sorted(u for u in build.TRANSLATION_UNITS if header in deps(u))
    assert users("msm_sort.h") == ["msm_g1.cpp"]
    assert users("msm_recode.h") == ["msm_g1.cpp", "zkamd.cpp"]
    # the umbrella is for the stand-alone benchmarks: no unit of the library includes it
    assert users("msm.h") == []
