"""Table multiples (csrc/msm_types.h MsmRecode, msm_recode.h msm_wnaf_mult, msm_point_kernels.h k_msm_build_table): a bound table holds, behind the 255 slices 2^k P
of every base, the slices of m 2^k P for the odd m = 3, 5, ..., and a scalar is recoded over the digits +- m b (b odd,
b < 2^(c-1)): digit m b goes into bucket b through the slice of m.  The group element a multiexp computes cannot change; what
can go wrong is the recoding (a digit that does not sum back to the scalar, a bucket past the histogram, a slice past the
table), the table (a wrong multiple, a chain started one doubling off) and the bookkeeping between the two passes of the sort.

(1) the recoding against integers: the hook zk_hook_recode (the kernels' msm_digits on single scalars, multiples and extra
    window bits given at run time) digit for digit against the rule restated here (_recode), and the invariants on their own.
(2) the table: entries (multiple, slice, base) of a G1 and a G2 group against the oracle's m 2^k P.
(3) multiexps over a table with multiples, both launch-set forms, against the oracle's sum and the result with one multiple;
    the selection bytes of MsmSelSet once with four multiples.
(4) proofs: four transfer statements on the GPU, ZKAMD_TABLE_MULTIPLES unset against = 1 and the oracle's discrete-log proof;
    in the emulation one statement through ensure_derived with two multiples.  The tables get their multiples with the key's
    first launch set of ZKAMD_TABLE_MULTIPLES_MIN jobs (129 by default: these tests set 1, and check once that four statements
    alone leave the key as it was).
(5) the out-of-memory fallback (ZKAMD_INJECT_TABLE_OOM): the key stays bound with one multiple and the proofs are the same.

Every case runs on the emulation build and, marked gpu, on the device through the hooks library."""
import ctypes as C
import functools

import numpy as np
import pytest

import zero_chain_amd as zk
from oracle import bls12_381 as bls
from oracle import synth
import helpers
import test_value_pairs as vp
import test_value_runs as vr

R = bls.R_MOD
NPOS = 255
DEFAULT_EXT = {1: 0, 2: 2, 4: 3, 8: 3}


def _max_digits(c):
    return 254 // c + 2          # msm_types.h msm_max_digits


# ----------------------------------------------------------------------------------------------
# (1) the recoding
# ----------------------------------------------------------------------------------------------
def _recode(s, c, n_mult, ext):
    """The rule, restated over integers: [(position, bucket, multiple index, negative)] in order of position"""
    if s == 0 or s >= R:
        return []
    flip = s > (R - 1) // 2
    k = R - s if flip else s
    mults = [2 * j + 1 for j in range(n_mult)]
    half, wide = 1 << (c - 1), c + ext
    out, pos = [], 0
    while k:
        z = (k & -k).bit_length() - 1
        k >>= z
        pos += z
        widths = range(wide, c - 1, -1) if n_mult > 1 and k.bit_length() > wide + 1 else [c]
        for w in widths:
            rho = k % (1 << w)
            hit = None
            for d in sorted((rho, rho - (1 << w)), key=abs):
                fits = [j for j, m in enumerate(mults) if abs(d) % m == 0 and abs(d) // m < half]
                if fits:
                    hit = (d, fits[0])
                    break
            if hit:
                break
        d, j = hit
        out.append((pos, abs(d) // mults[j], j, (d < 0) != flip))
        k = (k - d) >> w
        pos += w
    return out


def _edge_scalars(c, ext):
    wide = c + ext
    out = [0, 1, 2, 3, R - 1, (R - 1) // 2, (R + 1) // 2, R, R + 1, (1 << 256) - 1]          # (the last three: not canonical)
    for k in (31, 32, 63, 64, 223, 224, 253):
        out += [1 << k, (1 << k) - 1, (1 << k) + 1]
    out += [(1 << 254) - 1, (1 << 253) - 1, (1 << 128) - 1, int("55" * 31, 16), int("aa" * 31, 16)]
    # the top of the scalar: values whose last digits fall where a wide step no longer fits, at every length around W + 1 ...
    for length in range(c - 1, wide + 5):
        out += [(1 << length) - 1, (1 << length) + 1, (1 << length) + (1 << (length - 1)) + 1, (3 << length) - 1]
    # ... and the same residuals below the top of a long scalar (above a long run of zeros; above a run of ones: with the carry)
    for length in range(c - 1, wide + 5):
        for low in (200, 232):
            top = ((1 << length) + 1) << low
            out += [top + 1, top - 1, top + (1 << 100) - 1]
    return [x for x in out if x < (1 << 256)]


@functools.lru_cache(maxsize=None)
def _uniform(n=2000):
    rng = synth.SplitMix64(2028)
    return [rng.field(R) for _ in range(n)]


def _hook_recode(lib, c, n_mult, ext, scalars):
    fn = lib.dll.zk_hook_recode
    fn.restype = C.c_int32
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    cap = _max_digits(c) + 2
    sc = zk.scalars_to_bytes(scalars)
    out = np.zeros(len(scalars) * cap * 4, dtype=np.uint32)
    cnt = np.zeros(len(scalars), dtype=np.uint32)
    lib.check(fn(c, n_mult, ext, len(scalars), sc.ctypes.data, cap, out.ctypes.data, cnt.ctypes.data))
    out = out.reshape(len(scalars), cap, 4)
    assert int(cnt.max()) <= _max_digits(c), (c, n_mult, int(cnt.max()))
    return [[tuple(int(x) for x in out[i, k]) for k in range(int(cnt[i]))] for i in range(len(scalars))]


def _check_recoding(lib, c, n_mult, ext):
    scalars = _edge_scalars(c, ext) + _uniform()
    got = _hook_recode(lib, c, n_mult, ext, scalars)
    plain = _hook_recode(lib, c, 1, 0, scalars) if n_mult > 1 else got
    total_digits, total_plain = 0, 0
    for s, digits, base in zip(scalars, got, plain):
        assert digits == [(p, b, j, int(neg)) for p, b, j, neg in _recode(s, c, n_mult, ext)], (c, n_mult, ext, hex(s))
        if s == 0 or s >= R:
            assert digits == []
            continue
        value = sum((-1 if neg else 1) * (2 * j + 1) * b << p for p, b, j, neg in digits)
        assert value == (s - R if s > (R - 1) // 2 else s), (c, n_mult, hex(s))
        assert all(b & 1 and b < (1 << (c - 1)) and j < n_mult and p <= 254 for p, b, j, _ in digits), (c, n_mult, hex(s))
        assert all(q[0] - p[0] >= c for p, q in zip(digits, digits[1:])), (c, n_mult, hex(s))
        assert len(digits) <= _max_digits(c)
        total_digits += len(digits)
        total_plain += len(base)
    if n_mult == 1:   # ... and one multiple is the width-c NAF: one odd digit below 2^(c-1) per window, no other multiple
        assert all(j == 0 for digits in got for _, _, j, _ in digits)
    elif ext == 0:   # (no wider window: the candidate of the smaller magnitude at w = c is the NAF digit itself)
        assert got == plain
    else:
        assert total_digits < total_plain, (c, n_mult, total_digits, total_plain)
    return total_digits, total_plain


RECODE_CASES = [(c, m, DEFAULT_EXT[m]) for c in (4, 7, 13, 14, 16) for m in (1, 2, 4, 8)] + [(13, 4, 2), (16, 8, 4), (7, 2, 0)]


@pytest.mark.parametrize("c,n_mult,ext", RECODE_CASES)
def test_recoding_against_integers(emu_lib, c, n_mult, ext):
    _check_recoding(emu_lib, c, n_mult, ext)


def test_recoding_model_digit_counts():
    """the restated rule alone, on the uniform scalars: the mean digits per scalar it predicts for the shipped widths - the
    figures the widths and the expected pair counts rest on"""
    sc = _uniform()[:500]
    for c, want in ((16, (15.4, 14.85, 14.3)), (13, (18.55, 17.8, 17.0))):
        for n_mult, w in zip((1, 2, 4), want):
            mean = sum(len(_recode(s, c, n_mult, DEFAULT_EXT[n_mult])) for s in sc) / len(sc)
            assert abs(mean - w) < 0.15, (c, n_mult, mean)


@pytest.mark.gpu
@pytest.mark.parametrize("c,n_mult,ext", RECODE_CASES)
def test_gpu_recoding_against_integers(gpu_hooks_lib, c, n_mult, ext):
    _check_recoding(gpu_hooks_lib, c, n_mult, ext)


# ----------------------------------------------------------------------------------------------
# (2) the table, (3) multiexps over it
# ----------------------------------------------------------------------------------------------
def _mult_msm(lib, group, c, n_mult, bases, scalars=None, mp=None, entries=None, sel=None, alt=None, sel_first=0, sel_n=0, alt_w=0,
              ext=None):
    """zk_hook_mult_msm: scalars = one list per job; entries = [(multiple index, slice, base)]"""
    fn = lib.dll.zk_hook_mult_msm
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    size = 96 if group == 1 else 192
    ext = DEFAULT_EXT[n_mult] if ext is None else ext
    bs = np.frombuffer(bases, dtype=np.uint8).copy()
    n_jobs = len(scalars) if scalars else 0
    n = len(scalars[0]) if scalars else 0
    sc = zk.scalars_to_bytes([x for job in scalars for x in job]) if scalars else None
    m = np.array(mp, dtype=np.int32) if scalars else None
    out = np.zeros(max(n_jobs, 1) * size, dtype=np.uint8)
    en = np.array(entries, dtype=np.uint32).reshape(-1) if entries else None
    eo = np.zeros(max(len(entries) if entries else 0, 1) * size, dtype=np.uint8)
    by = np.array(sel, dtype=np.uint8) if sel is not None else None
    al = np.array(alt, dtype=np.int32) if sel is not None else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    lib.check(fn(group, c, n_mult, ext, len(bases) // size, bs.ctypes.data, n_jobs, n, ptr(sc), ptr(m), ptr(by), ptr(al), sel_first, sel_n,
                 alt_w, out.ctypes.data, len(entries) if entries else 0, ptr(en), eo.ctypes.data))
    return ([out[size * p:size * (p + 1)].tobytes() for p in range(n_jobs)],
            [eo[size * t:size * (t + 1)].tobytes() for t in range(len(entries) if entries else 0)])


def _encode(group, k):
    if k % R == 0:
        return bls.g1_uncompressed(None) if group == 1 else bls.g2_uncompressed(None)
    return helpers.g1_of(k) if group == 1 else helpers.g2_of(k)


@functools.lru_cache(maxsize=None)
def _bases(group, n, identity):
    rng = synth.SplitMix64(500 + group)
    dlog = [3 + rng.field(1 << 20) for _ in range(n)]
    dlog[identity] = 0
    return dlog, b"".join(_encode(group, k) for k in dlog)


def _check_table(lib, group, n_bases, n_mult):
    dlog, bases = _bases(group, n_bases, 2)
    entries = [(j, k, i) for j in range(n_mult) for k in (0, 1, 127, 254) for i in range(n_bases)]
    _, got = _mult_msm(lib, group, 6, n_mult, bases, entries=entries)
    for (j, k, i), g in zip(entries, got):
        assert g == _wanted_entry(group, dlog[i] * (2 * j + 1) << k), (group, j, k, i)


@functools.lru_cache(maxsize=None)
def _wanted_entry(group, k):
    return _encode(group, k)


def test_table_entries_g1(emu_lib):
    _check_table(emu_lib, 1, 8, 8)


def test_table_entries_g2(emu_lib):
    _check_table(emu_lib, 2, 4, 4)


@pytest.mark.gpu
def test_gpu_table_entries(gpu_hooks_lib):
    _check_table(gpu_hooks_lib, 1, 8, 8)
    _check_table(gpu_hooks_lib, 2, 4, 4)


N_BASES, N_SLOTS = 48, 60


@functools.lru_cache(maxsize=None)
def _jobs(n_jobs):
    """the map (repeated bases, one slot mapped out, base 2 the identity) and n_jobs scalar vectors: the first and the last
    job carry the edge values of the recoding"""
    rng = synth.SplitMix64(77 + n_jobs)
    mp = list(range(N_BASES)) + [k % 12 for k in range(N_SLOTS - N_BASES)]
    mp[9] = -1
    edge = [0, 1, 2, 3, R - 1, (R - 1) // 2, (R + 1) // 2, 1 << 31, (1 << 32) - 1, (1 << 64) + 1, (1 << 223) - 1, (1 << 224) + 1,
            (1 << 253) + 1, (1 << 254) - 1, (1 << 13) + 1, (1 << 20) - 1]
    jobs = []
    for p in range(n_jobs):
        sc = [rng.field(R) for _ in range(N_SLOTS)]
        if p in (0, n_jobs - 1):
            sc[20:20 + len(edge)] = edge
        jobs.append(sc)
    return mp, jobs


@functools.lru_cache(maxsize=None)
def _wanted_sums(n_jobs):
    dlog, _ = _bases(1, N_BASES, 2)
    mp, jobs = _jobs(n_jobs)
    return [_encode(1, sum(s * dlog[m] for s, m in zip(sc, mp) if m >= 0) % R) for sc in jobs]


def _check_multiexps(lib, c, n_jobs):
    _, bases = _bases(1, N_BASES, 2)
    mp, jobs = _jobs(n_jobs)
    want = _wanted_sums(n_jobs)
    one = None
    for n_mult in (1, 2, 4):
        got, _ = _mult_msm(lib, 1, c, n_mult, bases, scalars=jobs, mp=mp)
        one = one or got
        assert got == want, (c, n_jobs, n_mult, [p for p in range(n_jobs) if got[p] != want[p]][:5])
        assert got == one


@pytest.mark.parametrize("n_jobs", [2, 130])   # (the batch form of a launch set starts above 128 jobs)
@pytest.mark.parametrize("c", [5, 8])
def test_multiexps_over_multiples(emu_lib, c, n_jobs):
    _check_multiexps(emu_lib, c, n_jobs)


def _check_multiexp_g2(lib):
    dlog, bases = _bases(2, 12, 2)
    rng = synth.SplitMix64(31)
    jobs = [[rng.field(R) for _ in range(12)] for _ in range(2)]
    jobs[0][:4] = [R - 1, 1, (R + 1) // 2, 0]
    for n_mult in (1, 4):
        got, _ = _mult_msm(lib, 2, 5, n_mult, bases, scalars=jobs, mp=list(range(12)))
        assert got == [_encode(2, sum(s * k for s, k in zip(sc, dlog)) % R) for sc in jobs], n_mult


def test_multiexp_g2_over_multiples(emu_lib):
    _check_multiexp_g2(emu_lib)


def _check_selection(lib):
    """the job of test_value_runs (b): 64 slots for 2 proofs, bytes 0, 2, 3, 4 and absent alternates, over four multiples"""
    dlog, bases, mp, alt, scalars, sel = vr._select_job()
    got, _ = _mult_msm(lib, 1, 7, 4, bases, scalars=scalars, mp=mp, sel=sel[0] + sel[1], alt=alt, sel_first=vr.SEL_FIRST, sel_n=vr.SEL_N,
                       alt_w=vr.ALT_W)
    for p in range(2):
        total = 0
        for i in range(vr.N_SLOTS):
            pos, k = mp[i], i - vr.SEL_FIRST
            if 0 <= k < vr.SEL_N and sel[p][k] >= 3:
                pos = alt[k * vr.ALT_W + sel[p][k] - 3]
            if pos >= 0:
                total += scalars[p][i] * dlog[pos]
        assert got[p] == helpers.g1_of(total), p


def test_selection_bytes_over_multiples(emu_lib):
    _check_selection(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("n_jobs", [2, 130])
@pytest.mark.parametrize("c", [5, 8])
def test_gpu_multiexps_over_multiples(gpu_hooks_lib, c, n_jobs):
    _check_multiexps(gpu_hooks_lib, c, n_jobs)


@pytest.mark.gpu
def test_gpu_multiexp_g2_and_selection_over_multiples(gpu_hooks_lib):
    _check_multiexp_g2(gpu_hooks_lib)
    _check_selection(gpu_hooks_lib)


# ----------------------------------------------------------------------------------------------
# (4) proofs, (5) the out-of-memory fallback
# ----------------------------------------------------------------------------------------------
def _bound(lib, params):
    fn = lib.dll.zk_hook_bound_multiples
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p]
    info = np.zeros(6, dtype=np.uint32)
    lib.check(fn(params._h, info.ctypes.data))
    return [int(x) for x in info]


def _prove(lib, r1, pk, sts, rs, after=None):
    """a fresh key per call: a key is bound to its circuit once, under the variables of that moment"""
    params = zk.Parameters.read(pk, checked=False, lib=lib)
    mats = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    try:
        proofs = [p.write() for p in zk.transfer_prove_batch(mats, params, sts, rs)]
        return proofs, (after(params) if after else None)
    finally:
        mats.close()
        params.close()


def _four_statements():
    import sys
    sys.path.insert(0, vp.ROOT)
    import bench
    from oracle import transfer_circuit as tc
    ws, rs, want = vp._transfer_wanted()
    seed, amount, fee, balance = bench.statement_params(3)
    ws = list(ws) + [tc.make_witness(seed, amount=amount, fee=fee, balance=balance)]
    rs = list(rs) + [(12345678901234567890123 % R, 98765432109876543210987 % R)]
    return zk.transfer_statements([tc.statement_dict(w) for w in ws]), rs, want


@pytest.mark.gpu
def test_gpu_four_transfer_statements(gpu_hooks_lib, monkeypatch):
    """the chunk form (split launch sets): the bytes under ZKAMD_TABLE_MULTIPLES unset, = 1 and = 2, and the oracle's
    discrete-log proofs of the first three; what the key was bound with each time"""
    lib = gpu_hooks_lib
    r1, _, P, pk = helpers.transfer_case(1)
    sts, rs, want = _four_statements()
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    monkeypatch.delenv("ZKAMD_TABLE_MULTIPLES", raising=False)
    monkeypatch.delenv("ZKAMD_TABLE_MULTIPLES_MIN", raising=False)
    alone, bound = _prove(lib, r1, pk, sts, rs, lambda p: _bound(lib, p))
    assert bound[:2] == [1, 1]                        # four statements are no batch: the key as it was
    monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES_MIN", "1")
    unset, bound = _prove(lib, r1, pk, sts, rs, lambda p: _bound(lib, p))
    assert bound[0] == bound[1] and bound[0] in (2, 4, 8)
    assert len(unset) == 4 and unset[:3] == want and unset == alone
    for m in (1, 2):
        monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES", str(m))
        got, bound = _prove(lib, r1, pk, sts, rs, lambda p: _bound(lib, p))
        assert bound[:2] == [m, m]
        assert got == unset, m


@pytest.mark.gpu
def test_gpu_table_out_of_memory_binds_one_multiple(gpu_hooks_lib, monkeypatch):
    lib = gpu_hooks_lib
    r1, _, P, pk = helpers.transfer_case(1)
    sts, rs, want = _four_statements()
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES", "4")
    monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES_MIN", "1")
    monkeypatch.setenv("ZKAMD_INJECT_TABLE_OOM", "1")
    got, bound = _prove(lib, r1, pk, sts, rs, lambda p: _bound(lib, p))
    assert bound[:2] == [1, 1]
    assert got[:3] == want
    monkeypatch.delenv("ZKAMD_INJECT_TABLE_OOM")
    again, bound = _prove(lib, r1, pk, sts, rs, lambda p: _bound(lib, p))
    assert bound[:2] == [4, 4] and again == got


def test_emulated_transfer_statement_two_multiples(emu_lib, monkeypatch):
    """One transfer statement through the chunk form of the emulation build with ZKAMD_TABLE_MULTIPLES=2 from the first set on: both
    bound tables get the slices of 3 P (MsmGroup::add_multiples), the three launch sets recode over them, and the bytes are the oracle's.  Slow like
    test_value_pairs.py::test_emulated_transfer_statement_chunk_form (the emulation binds the key in minutes)."""
    from oracle import transfer_circuit as tc
    monkeypatch.setenv("ZKAMD_SPLIT_MIN", "1")
    monkeypatch.setenv("ZKAMD_FOLD_IN_MSM_MAX", "0")
    monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES", "2")
    monkeypatch.setenv("ZKAMD_TABLE_MULTIPLES_MIN", "1")
    r1, _, P, pk = helpers.transfer_case(1)
    ws, rs, want = vp._transfer_wanted()
    sts = zk.transfer_statements([tc.statement_dict(ws[0])])
    got, bound = _prove(emu_lib, r1, pk, sts, rs[:1], lambda p: _bound(emu_lib, p))
    assert bound[:2] == [2, 2]
    assert got == want[:1]
