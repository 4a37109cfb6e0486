"""Which constraint an assignment breaks, checked by the library (zk_r1cs_check_batch, zk_transfer_check_batch,
zk_anonymous_check_batch, zk_r1cs_stage; csrc/r1cs_check.h) against Python integers (tests/r1cs_check_cases.py `reference`:
<A_j, z> * <B_j, z> mod r against <C_j, z>, the lowest failing row and the count).  Every comparison is exact and none needs a
proving key.  Every case runs on the x86 emulation build and, marked gpu, on the product library.  The anonymous-circuit cases
run the host witness engine on the emulation build too: three statements take a few seconds there."""
import ctypes as C

import pytest

import r1cs_check_cases as rc
from oracle import anonymous_circuit as ac
from oracle import transfer_circuit as tc

LIBS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
# (library, witness engine): the witness kernels only where there is a GPU
ENGINES = [("emu", "host"), pytest.param("gpu", "host", marks=pytest.mark.gpu), pytest.param("gpu", "gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=LIBS)
def lib(request):
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "gpu_lib")


_loaded = {}   # (library, what) -> ConstraintMatrices: loaded once, shared by the tests


def matrices(lib, system, broken=None):
    import zero_chain_amd as zk
    key = (lib.path, system.name, broken)
    if key not in _loaded:
        cons = system.constraints if broken is None else system.broken(broken)
        _loaded[key] = (zk.ConstraintMatrices(system.n_in, system.n_aux, cons, lib=lib), cons)
    return _loaded[key]


def builtin(lib, circuit):
    import zero_chain_amd as zk
    key = (lib.path, circuit, None)
    if key not in _loaded:
        _loaded[key] = getattr(zk.ConstraintMatrices, circuit)(lib=lib)
    return _loaded[key]


def test_reference_agrees_with_the_oracle():
    rc.check_reference_against_oracle()


@pytest.mark.parametrize("montgomery", [False, True])
@pytest.mark.parametrize("which", range(3))
def test_synthetic_assignments_one_by_one(lib, which, montgomery):
    """the satisfying assignment, the last aux variable + 1, z_0 = 2 (flag set, rows as the integers say), one more variable + 1 -
    and the satisfying assignment against the system with one row in the middle, then the very last row, made to fail alone"""
    s = rc.systems()[which]
    form = rc.to_mont if montgomery else list
    m, cons = matrices(lib, s)
    for name, z in s.variants().items():
        want = rc.reference(cons, z)
        assert m.check([form(z)], montgomery=montgomery) == [want], name
        if name == "satisfying":
            assert want == (None, 0, True)
        if name == "one_is_two":
            assert want[2] is False
    n_con = len(s.constraints)
    for j in sorted({n_con // 2, n_con - 1}):
        m, cons = matrices(lib, s, broken=j)
        assert rc.reference(cons, s.z) == (j, 1, True)
        assert m.check([form(s.z)], montgomery=montgomery) == [(j, 1, True)]


@pytest.mark.parametrize("n", [1, 3, 65, 130, 255, 256, 321])
@pytest.mark.parametrize("which", range(3))
def test_synthetic_batches(lib, which, n):
    """broken assignments at positions 0, 63, 64 and the last one of a batch: both lane mappings cross a wave there.  From 256
    assignments on the library runs the lanes of a wave across proofs (zkamd.cpp R1CS_CHECK_LANE_MIN): 255 and 256 stand on
    either side, and 321 leaves one lane in the last group of 64."""
    s = rc.systems()[which]
    m, cons = matrices(lib, s)
    v = s.variants()
    zs = [v["satisfying"]] * n
    for pos, name in ((0, "last_aux"), (63, "one_is_two"), (64, "first_aux"), (255, "first_aux"), (256, "one_is_two"), (n - 1, "last_aux")):
        if pos < n:
            zs[pos] = v[name]
    want = {name: rc.reference(cons, z) for name, z in v.items()}
    expect = [next(want[name] for name, z in v.items() if z is zs[i]) for i in range(n)]
    assert any(e[1] for e in expect)
    assert m.check(zs) == expect
    # ... and against the system whose last row fails for every assignment that satisfied it
    m, cons = matrices(lib, s, broken=len(s.constraints) - 1)
    assert m.check(zs) == [rc.reference(cons, z) for z in zs]


def test_three_chunks(lib, monkeypatch):
    monkeypatch.setenv("ZKAMD_BATCH_CHUNK", "8")
    s = rc.systems()[2]
    m, cons = matrices(lib, s)
    v = s.variants()
    names = list(v)
    zs = [v[names[(5 * i) % len(names)]] for i in range(19)]
    assert m.check(zs) == [rc.reference(cons, z) for z in zs]


def test_empty_batch_and_a_scalar_equal_to_r(lib):
    import zero_chain_amd as zk
    s = rc.systems()[1]
    m, _ = matrices(lib, s)
    assert m.check([]) == []
    for montgomery in (False, True):
        z = list(s.z)
        z[s.n_in + 2] = rc.R
        with pytest.raises(zk.ZkError) as e:
            m.check([s.z, z], montgomery=montgomery)
        assert e.value.variant == "InvalidArgument" and "canonical" in str(e.value)


# ---- the transfer circuit
@pytest.mark.parametrize("which,engine", ENGINES)
def test_transfer_statements(request, monkeypatch, which, engine):
    """remaining balance + 1 breaks the two rows of the balance equation and nothing else"""
    import zero_chain_amd as zk
    lib = request.getfixturevalue("emu_lib" if which == "emu" else "gpu_lib")
    monkeypatch.setenv("ZKAMD_WITNESS", engine)
    ws, want = rc.transfer_statement_cases()
    assert want == [(None, 0), (15649, 2), (None, 0)]
    sts = zk.transfer_statements([tc.statement_dict(w) for w in ws])
    assert zk.transfer_check(builtin(lib, "transfer_circuit"), sts) == [w + (True,) for w in want]
    assert zk.transfer_check(builtin(lib, "transfer_circuit"), zk.transfer_statements([])) == []


def test_transfer_amount_outside_the_range_gadget(lib):
    z, want = rc.transfer_u32_max_case()
    assert want == (61, 1)
    assert builtin(lib, "transfer_circuit").check([z]) == [want + (True,)]


def stages_of(m, n_con):
    out, c = [], 0
    while c < n_con:
        stage, first, count, name = m.stage(c)
        assert first == c and count > 0 and name
        assert m.stage(c + count - 1) == (stage, first, count, name)
        out.append((stage, first, count, name))
        c += count
    assert c == n_con
    assert [s[0] for s in out] == list(range(len(out)))
    return out


def test_transfer_stages(lib):
    import zero_chain_amd as zk
    m = builtin(lib, "transfer_circuit")
    stages = stages_of(m, 19974)
    assert len(stages) > 20 and len({s[3] for s in stages}) == len(stages)
    a, b = m.stage(15649), m.stage(15650)
    assert a == b and a[1:3] == (15649, 2) and "balance" in a[3]
    assert m.stage(61)[1] == 0 and "amount" in m.stage(61)[3]
    r1 = rc.transfer_constraints()
    plain = zk.ConstraintMatrices(r1.n_in, r1.n_aux, r1.constraints, lib=lib)
    assert plain.stage(15649) == (None, 0, 19974, "")
    # ... whose rows are the built-in system's: the same verdict for the same assignment
    z, want = rc.transfer_u32_max_case()
    assert plain.check([z]) == [want + (True,)]
    plain.close()
    assert zk.transfer_r1cs_fingerprint(lib)[0] == tc.REFERENCE_HASH


# ---- the anonymous circuit
@pytest.mark.parametrize("which,engine", ENGINES)
def test_anonymous_statements(request, monkeypatch, which, engine):
    import zero_chain_amd as zk
    lib = request.getfixturevalue("emu_lib" if which == "emu" else "gpu_lib")
    monkeypatch.setenv("ZKAMD_WITNESS", engine)
    ws, want = rc.anonymous_statement_cases()
    assert want[0] == (None, 0, True) and want[1][1] > 0 and want[2][1] > 0
    sts = zk.anonymous_statements([ac.statement_dict(w) for w in ws])
    assert zk.anonymous_check(builtin(lib, "anonymous_circuit"), sts) == want


def test_anonymous_stages(lib):
    m = builtin(lib, "anonymous_circuit")
    stages = stages_of(m, 50514)
    _, want = rc.anonymous_statement_cases()
    for first_bad, _, _ in want[1:]:
        assert any(s[1] <= first_bad < s[1] + s[2] for s in stages)


# ---- refusals
def test_refusals(lib):
    import zero_chain_amd as zk
    transfer = builtin(lib, "transfer_circuit")
    ws, _ = rc.anonymous_statement_cases()
    sts = zk.anonymous_statements([ac.statement_dict(ws[0])])
    with pytest.raises(zk.ZkError) as e:
        zk.anonymous_check(transfer, sts)
    assert e.value.variant == "InvalidArgument" and "anonymous-transfer circuit" in str(e.value)
    s = rc.systems()[1]
    m, _ = matrices(lib, s)
    w = zk.scalars_to_bytes(s.z)
    with pytest.raises(zk.ZkError) as e:
        lib.check(lib.zk_r1cs_check_batch(m._h, 1, w.ctypes.data_as(C.c_void_p), 0, None))
    assert e.value.variant == "InvalidArgument" and "null" in str(e.value)
    tws, _ = rc.transfer_statement_cases()
    tsts = zk.transfer_statements([tc.statement_dict(tws[0])])
    with pytest.raises(zk.ZkError) as e:
        lib.check(lib.zk_transfer_check_batch(transfer._h, 1, tsts, None))
    assert e.value.variant == "InvalidArgument"
    for bad in (len(s.constraints), 0xFFFFFFFF):
        with pytest.raises(zk.ZkError) as e:
            m.stage(bad)
        assert e.value.variant == "InvalidArgument"
    with pytest.raises(zk.ZkError):
        transfer.stage(19974)
    # a malformed statement: the status, the message and the index of the prove entries (statement_route.h)
    d = tc.statement_dict(tws[0])
    bad = zk.transfer_statements([d, dict(d, g_epoch=bytes([0xff] * 32))])
    with pytest.raises(zk.ZkError) as e:
        zk.transfer_check(transfer, bad)
    assert e.value.variant == "InvalidArgument" and "statement 1" in str(e.value) and "g_epoch" in str(e.value)
