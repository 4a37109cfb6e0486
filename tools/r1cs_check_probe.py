#!/usr/bin/env python3
"""What the constraint check costs (csrc/r1cs_check.h), beside the prover's row evaluations on the same assignments in the
same process: ONE JSON line.

  kernel ms (HIP events, zk_profile_*; three warm calls discarded, median of five with min and max) on a resident chunk of
  1024 transfer assignments and of 512 anonymous ones, left in the circuit's workspace by a check call:
    r1cs_check_rows     k_r1cs_check, one thread per (row, proof): k_r1cs_eval's mapping
    r1cs_check_proofs   k_r1cs_check, the lanes of a wave across 64 proofs of one row
    r1cs_eval           k_r1cs_eval, as zk_prove_batch_witness launches it
  and k_r1cs_check under both mappings on the first 16, 64, 128, 256 and 512 of the transfer assignments (medians): where the
  mappings cross, which is what R1CS_CHECK_LANE_MIN (zkamd.cpp) is set by
  wall ms (host clock round the entry, one warm call discarded, median of three), recorded only:
    zk_transfer_check_batch for 1, 64 and 1024 statements; zk_transfer_prove_batch for the same 1024
The mapping is forced, and the two kernels launched alone, through the entries of the hooks library (libzkamd_hooks.so).
The 512 anonymous statements are four distinct ones repeated: the rows' work does not depend on the values.
Usage: python tools/r1cs_check_probe.py [out.json]     (the committed run: profiles/r26_r1cs_check.json)
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ZK_LIB_FLAVOR"] = "hooks"

WARM, REPS = 3, 5
ROWS, PROOFS, AUTO = 0, 1, -1


def main():
    import importlib.util
    import zero_chain_amd as zk
    from zero_chain_amd import _lib
    import helpers
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    lib = zk.load_library()
    for name in ("zk_hook_r1cs_check_mapping", "zk_hook_r1cs_check_resident", "zk_hook_r1cs_eval_resident"):
        getattr(lib.dll, name).restype = C.c_int32
    lib.dll.zk_hook_r1cs_check_mapping.argtypes = [C.c_int]
    lib.dll.zk_hook_r1cs_check_resident.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.R1csVerdict)]
    lib.dll.zk_hook_r1cs_eval_resident.argtypes = [C.c_void_p, C.c_size_t]

    def stat(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

    def kernel_ms(name, call):
        out = []
        for rep in range(WARM + REPS):
            with zk.KernelTimer(lib) as t:
                call()
                launches, ms = t.get(name)
            assert launches == 1, (name, launches)
            if rep >= WARM:
                out.append(ms)
        return stat(out)

    def resident(mats, n):
        verdicts = (_lib.R1csVerdict * n)()
        res = {}
        for key, mapping in (("r1cs_check_rows", ROWS), ("r1cs_check_proofs", PROOFS)):
            lib.check(lib.dll.zk_hook_r1cs_check_mapping(mapping))
            res[key] = kernel_ms("r1cs_check", lambda: lib.check(lib.dll.zk_hook_r1cs_check_resident(mats._h, n, verdicts)))
            assert all(v.first_bad == _lib.ZK_R1CS_SATISFIED and v.n_bad == 0 and v.flags == 0 for v in verdicts), key
        lib.check(lib.dll.zk_hook_r1cs_check_mapping(AUTO))
        res["r1cs_eval"] = kernel_ms("r1cs_eval", lambda: lib.check(lib.dll.zk_hook_r1cs_eval_resident(mats._h, n)))
        for key in ("r1cs_check_rows", "r1cs_check_proofs"):
            res[key + "_over_eval"] = round(res[key]["median"] / res["r1cs_eval"]["median"], 4)
        return res

    def wall_ms(call):
        out = []
        for rep in range(1 + 3):
            t0 = time.perf_counter()
            call()
            if rep >= 1:
                out.append((time.perf_counter() - t0) * 1e3)
        return stat(out)

    line = {"probe": "r1cs_check", "warm": WARM, "reps": REPS, "check_rows_per_wave": 32}
    os.environ["ZKAMD_WITNESS"] = "gpu"   # the resident chunk: one launch set of the witness kernels, in slot 0
    mats = zk.ConstraintMatrices.transfer_circuit(lib=lib)
    items = bench.make_statements_native(zk, lib, 0, 1024)
    sts = zk.transfer_statements(items)
    assert zk.transfer_check(mats, sts) == [(None, 0, True)] * 1024
    line["transfer_1024"] = resident(mats, 1024)
    # where the two mappings cross: the first np assignments of the same resident chunk
    cross = {}
    verdicts = (_lib.R1csVerdict * 1024)()
    for n in (16, 64, 128, 256, 512):
        cross[str(n)] = {}
        for key, mapping in (("rows", ROWS), ("proofs", PROOFS)):
            lib.check(lib.dll.zk_hook_r1cs_check_mapping(mapping))
            cross[str(n)][key] = kernel_ms("r1cs_check", lambda: lib.check(lib.dll.zk_hook_r1cs_check_resident(mats._h, n, verdicts)))["median"]
    lib.check(lib.dll.zk_hook_r1cs_check_mapping(AUTO))
    line["transfer_check_ms_by_assignments"] = cross

    anon = zk.ConstraintMatrices.anonymous_circuit(lib=lib)
    distinct = [bench._make_anonymous(i) for i in range(4)]
    asts = zk.anonymous_statements([distinct[i % 4] for i in range(512)])
    assert zk.anonymous_check(anon, asts) == [(None, 0, True)] * 512
    line["anonymous_512"] = resident(anon, 512)
    anon.close()

    del os.environ["ZKAMD_WITNESS"]       # the library's own choice of the engine, as a caller gets it
    wall = {}
    for n in (1, 64, 1024):
        part = zk.transfer_statements(items[:n])
        wall["transfer_check_%d" % n] = wall_ms(lambda: zk.transfer_check(mats, part))
    params = zk.Parameters.read(zk.generate_parameters(mats, *helpers.TOXIC), checked=False, lib=lib)
    rs = [(3 + i, 5 + i) for i in range(1024)]
    wall["transfer_prove_1024"] = wall_ms(lambda: zk.transfer_prove_batch(mats, params, sts, rs))
    line["wall_ms"] = wall
    text = json.dumps(line)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
