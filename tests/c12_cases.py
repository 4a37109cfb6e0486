"""Cases for the Fq12 arithmetic on twelve rows (csrc/coop_pairing.cpp: c12_operand, c12_mul, c12_line, c12_cyc_sqr,
c12_mul_fq2 / c12_frob, c12_conj, c12_exp_x, c12_inv, c12_pos), shared by the emulation (CPU) and the GPU tests of
tests/test_c12_ops.py.  Every op of the test hook zk_hook_c12_op gets cases whose limbs the builder chooses one by one - the
operands, limb forms and margins of tests/field_cases.py - and every output row is compared with Python integers and with the
contract the header states for the function.

The reference knows nothing of the kernel's formulas: an Fq12 element is a polynomial of degree < 6 in w over Fq2, multiplied
schoolbook modulo w^6 - (1 + u) (mul12); the cyclotomic square is the plain square; a Frobenius map is a^(q^j) by
exponentiation for four elements per j and the coefficient-wise form, validated by those four, for the rest; the Frobenius
constants are xi^(k (q^j - 1) / 6) computed here; an inverse is checked by multiplying back to 1.  Residues are compared after
removing the Montgomery radix 2^392.

What the magnitude comments of coop_pairing.cpp state and these cases reach (units of p): components of c12_mul,
c12_cyc_sqr, c12_mul_fq2 operands below 4, a line's constant term below 64 and its two products below 2, the g of
c12_mul_fq2 below 2, the operand of c12_conj below 2 and its result below 3 - on all twelve rows at once and on one row
with the rest small, within 2 EPS below the bound, in limb forms with limbs at 2^28 + 8, runs of 2^28 - 1 and zeros."""
import ctypes as C
import functools
import os
import re

import numpy as np

import coop_cases as cc
import field_cases as fc
from field_cases import EPS, MASK, P, R392, RINV, W, WK, exact, operands, pick, sprinkled, val, weak
from oracle import pairing as opair
from oracle import synth
from oracle.bls12_381 import BLS_X

# the order of ZK_HK_C12_OPS in csrc/coop_pairing.cpp: (name, slots in, words out per case)
OPS = [("C12_MUL", 24, 192), ("C12_SQR", 12, 192), ("C12_LINE", 18, 192), ("C12_CYC_SQR", 12, 192), ("C12_MUL_FQ2_J0", 36, 192),
       ("C12_MUL_FQ2_J1", 36, 192), ("C12_MUL_FQ2_J2", 36, 192), ("C12_CONJ", 12, 192), ("C12_CONJ_MUL", 24, 192), ("C12_EXP_X", 12, 192),
       ("C12_INV", 36, 192), ("C12_EXPORT", 12, 144)]
OP_NAMES = [n for n, _, _ in OPS]
OP_CODE = {n: i for i, n in enumerate(OP_NAMES)}
MAX_CASES = {"C12_EXP_X": 64, "C12_INV": 64}


def ops_of_the_c_source(table="ZK_HK_C12_OPS", unit="coop_pairing.cpp"):
    """[(name, numbers...)] of an X-macro table of the C source"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zero-chain_amd", "csrc", unit)).read()
    body = re.search(r"#define %s\(X\)(.*?)\n(?!\s+X\()" % table, src.replace("\\\n", "\n"), flags=re.S).group(1)
    return [(m.group(1),) + tuple(int(x) for x in m.group(2).split(",")) for m in re.finditer(r"X\((\w+),\s*([\d,\s]+)\)", body)]


# ------------------------------------------------------------------------------------------------ Fq12 in integers
ZERO2, ONE2, XI = (0, 0), (1, 0), (1, 1)
ONE12 = (ONE2,) + (ZERO2,) * 5
ZERO12 = (ZERO2,) * 6


def mul2(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def pow2(a, e):
    r = ONE2
    for bit in bin(e)[2:]:
        r = mul2(r, r)
        if bit == "1":
            r = mul2(r, a)
    return r


def mul12(a, b):
    """schoolbook: the 36 products of the coefficients, then w^(6 + k) = (1 + u) w^k"""
    acc = [[0, 0] for _ in range(11)]
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            acc[i + j][0] += x[0] * y[0] - x[1] * y[1]
            acc[i + j][1] += x[0] * y[1] + x[1] * y[0]
    out = []
    for k in range(6):
        c0, c1 = acc[k]
        if k < 5:
            h0, h1 = acc[k + 6]
            c0, c1 = c0 + h0 - h1, c1 + h0 + h1
        out.append((c0 % P, c1 % P))
    return tuple(out)


def conj12(a):
    """a^(q^6): w -> -w"""
    return tuple(((-c[0]) % P, (-c[1]) % P) if k & 1 else c for k, c in enumerate(a))


def pow12(a, e):
    r = ONE12
    for bit in bin(e)[2:]:
        r = mul12(r, r)
        if bit == "1":
            r = mul12(r, a)
    return r


@functools.lru_cache(maxsize=None)
def gamma(j, k):
    """xi^(k (q^j - 1) / 6): what w^k picks up under a -> a^(q^j)"""
    assert (P ** j - 1) % 6 == 0
    return pow2(XI, k * (P ** j - 1) // 6) if j else ONE2


def conj2j(c, j):
    return (c[0], (-c[1]) % P) if j & 1 else c


def frob12(a, j):
    """the coefficient-wise form of a^(q^j) (validated against the exponentiation by frobenius_is_validated)"""
    return tuple(mul2(conj2j(c, j), gamma(j, k)) for k, c in enumerate(a))


def rand12(rng):
    return tuple((rng.field(P), rng.field(P)) for _ in range(6))


@functools.lru_cache(maxsize=None)
def frobenius_is_validated():
    rng = synth.SplitMix64(307)
    for j in (1, 2):
        for a in [rand12(rng) for _ in range(3)] + [tuple((0, 1) if k == 5 else ZERO2 for k in range(6))]:
            assert frob12(a, j) == pow12(a, P ** j), j
    return True


@functools.lru_cache(maxsize=None)
def cyclotomic_base():
    """t^((q^6 - 1)(q^2 + 1)) of random t, by exponentiation"""
    rng = synth.SplitMix64(311)
    out = [pow12(rand12(rng), (P ** 6 - 1) * (P ** 2 + 1)) for _ in range(3)]
    for g in out:
        assert g != ONE12 and mul12(g, conj12(g)) == ONE12          # norm 1 over Fq6: conj is the inverse
    return out


def cyclotomic(n):
    """n elements of the cyclotomic subgroup: 1, the three of cyclotomic_base, their conjugates, products and small powers"""
    b = cyclotomic_base()
    out = [ONE12] + b + [conj12(g) for g in b]
    i = 0
    while len(out) < n:
        out.append(mul12(out[1 + i % (len(out) - 1)], pow12(b[i % 3], 2 + i)))
        i += 1
    return out[:n]


def plain12(slots):
    """12 slots (row 2 k + c) -> the element without the Montgomery radix"""
    c = [val(s) * RINV % P for s in slots]
    return tuple((c[2 * k], c[2 * k + 1]) for k in range(6))


# ------------------------------------------------------------------------------------------------ operands
def edge_forms(bound, rng):
    """Limb vectors within 2 EPS below bound p (and at most bound p - EPS): limbs 12 and 13 fixed, the twelve low limbs - all of
    which lie below EPS - in the forms carries go wrong on."""
    hi = ((bound * P - EPS) >> 336) - 2
    base = exact(hi << 336)
    assert base[:12] == [0] * 12
    lows = [[WK] * 12, [MASK] * 12, [0] * 12, [WK] + [MASK] * 11, [rng.below(W), WK] + [MASK] * 10, [MASK] * 5 + [WK] + [MASK] * 6, [WK, 0] * 6,
            [W] + [MASK] * 11, [MASK] * 11 + [WK], [0] * 11 + [WK], [rng.below(W) for _ in range(12)], [8, W + 8, MASK, MASK, 0, 0, W, MASK, 1, W + 7, MASK, MASK]]
    out = [low + base[12:] for low in lows]
    for l in out:
        assert bound * P - 2 * EPS <= val(l) <= bound * P - EPS and all(x <= WK for x in l[:13])
    return out


@functools.lru_cache(maxsize=None)
def carry_pool():
    rng = synth.SplitMix64(397)
    pool = [t for t, _ in cc.carry_runs(rng, False)] + [sprinkled(rng.field(P), rng) for _ in range(30)]
    pool = [t for t in pool if val(t) <= 2 * P - EPS]          # (the runs that reach limb 13 are values above 2 p)
    assert len(pool) > 100
    return pool


class Lift:
    """plain residues -> slots: v 2^392 mod p + m p below bound p, m and the limb form (exact / weak) chosen case by case"""

    def __init__(self, seed):
        self.rng = synth.SplitMix64(seed)

    def comp(self, v, bound, m=None):
        r = self.rng
        m = (bound - 1 if r.below(2) else r.below(bound)) if m is None else m
        s = v * R392 % P + m * P
        return weak(s) if r.below(2) else exact(s)

    def elem(self, f, bound, m=None):
        return [self.comp(f[k][c], bound, m) for k in range(6) for c in range(2)]

    def edge(self, bound):
        return pick(edge_forms(bound, self.rng), self.rng.below(1000))

    def edges(self, bound, n=12):
        return [self.edge(bound) for _ in range(n)]

    def small(self, n=12):
        r = self.rng
        return [[exact(0), exact(1), exact(r.below(1 << 30)), exact(r.field(P)), weak(r.field(P))][r.below(5)] for _ in range(n)]

    def runs(self, n=12):
        """weak limbs below 2 p with a generated carry under runs of 2^28 - 1 (coop_cases.carry_runs), and sprinkled values"""
        return [pick(carry_pool(), self.rng.below(10000)) for _ in range(n)]

    def one_edge(self, bound, row, n=12):
        s = self.small(n)
        s[row] = self.edge(bound)
        return s


def structured(rng):
    """(what, element): 0, 1, the twelve basis elements (a one, and a random value, in one component), elements of the Fq2 and
    Fq6 subfields, random elements"""
    r2 = lambda: (rng.field(P), rng.field(P))
    out = [("zero", ZERO12), ("one", ONE12)]
    for i in range(12):
        for v in (1, rng.field(P)):
            out.append(("basis %d" % i, tuple(((v, 0) if i % 2 == 0 else (0, v)) if k == i // 2 else ZERO2 for k in range(6))))
    out += [("Fq2", (r2(),) + (ZERO2,) * 5) for _ in range(2)]
    out += [("Fq6", tuple(r2() if k % 2 == 0 else ZERO2 for k in range(6))) for _ in range(2)]
    out += [("random", rand12(rng)) for _ in range(4)]
    return out


def limb_forms_present(cases):
    """limbs at 2^28 + 8, runs of 2^28 - 1 and zero limbs all appear among the operands of the launch"""
    slots = [s for c in cases for s in c]
    assert any(WK in s[:13] for s in slots) and any(0 in s[:13] for s in slots)
    assert any(s[j] == MASK and s[j + 1] == MASK and s[j + 2] == MASK for s in slots for j in range(11))


def bounded(slots, bound):
    assert all(val(s) <= bound * P - EPS and all(x <= WK for x in s[:13]) for s in slots), bound


# ------------------------------------------------------------------------------------------------ the hook
def run(lib, name, cases):
    """cases: one list of input slots per case.  -> per case the 12 output slots (14 limbs each), or the 144 words of C12_EXPORT"""
    code = OP_CODE[name]
    _, ni, wo = OPS[code]
    n = len(cases)
    assert cases and all(len(c) == ni for c in cases), name
    assert (100 <= n <= 300) if name not in MAX_CASES else n <= MAX_CASES[name], (name, n)
    a = np.zeros((n, ni, 16), dtype=np.uint32)
    for i, c in enumerate(cases):
        for s, slot in enumerate(c):
            a[i, s, :14] = slot
    a[:, :, 14:] = 0xdeadbeef          # the pad words are ignored
    out = np.full((n, wo), 0xa5a5a5a5, dtype=np.uint32)
    fn = lib.dll.zk_hook_c12_op
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.check(fn(code, n, a.ctypes.data, out.ctypes.data))
    if name == "C12_EXPORT":
        return [[int(x) for x in out[i]] for i in range(n)]
    out = out.reshape(n, 12, 16)
    assert not out[:, :, 14:].any(), name          # pad words are zero
    return [[[int(x) for x in out[i, s, :14]] for s in range(12)] for i in range(n)]


def assert_rows(o, want, bound, what):
    """every output row: weakly normalised, below bound p, exactly the reference's residue"""
    got = plain12(o)
    for r in range(12):
        fc.assert_weak(o[r], (what, r))
        assert val(o[r]) < bound * P, (what, r, float(fc.ratio(o[r])))
        assert got[r // 2][r % 2] == want[r // 2][r % 2], (what, r)


# ------------------------------------------------------------------------------------------------ products
def operand_pairs(seed, bf, bg):
    """(f slots, g slots) for a product whose first operand's components lie below bf p and the second's below bg p"""
    L = Lift(seed)
    rng = L.rng
    st = structured(rng)
    rnd = [e for w, e in st if w == "random"]
    pairs = []
    for i, (what, e) in enumerate(st):                      # 0, 1, every basis element, the subfields: on either side
        pairs.append((e, rnd[i % len(rnd)]))
        pairs.append((rnd[i % len(rnd)], e))
    basis = [e for w, e in st if w.startswith("basis")]
    pairs += [(basis[2 * i], basis[2 * j + 1]) for i in range(12) for j in range(12) if (5 * i + j) % 4 == 0]   # every wrap, every sign
    sub = [e for w, e in st if w in ("Fq2", "Fq6")]
    pairs += [(a, b) for a in sub for b in sub[::2]]
    pairs += [(f, conj12(f)) for f in rnd] + [(conj12(f), f) for f in rnd[:2]]
    pairs += [(ZERO12, ZERO12), (ONE12, ONE12)]
    cases = [L.elem(f, bf) + L.elem(g, bg) for f, g in pairs]
    cases += [L.elem(f, bf, bf - 1) + L.elem(g, bg, bg - 1) for f, g in pairs[::9]]          # the top representative everywhere
    for _ in range(24):                                      # all twenty-four components at the edge
        cases.append(L.edges(bf) + L.edges(bg))
    for row in range(12):                                    # one row at the edge, the rest small
        cases.append(L.one_edge(bf, row) + L.small())
        cases.append(L.small() + L.one_edge(bg, row))
        cases.append(L.one_edge(bf, row) + L.edges(bg))
    cases += [L.runs() + L.runs() for _ in range(8)]
    for c in cases:
        bounded(c[:12], bf)
        bounded(c[12:], bg)
    limb_forms_present(cases)
    return cases


def check_mul(lib, name):
    if name == "C12_SQR":
        cases = [c[:12] for c in operand_pairs(331, 4, 4)] + [c[12:] for c in operand_pairs(331, 4, 4)[::3]]
        cases = cases[:300]
        ref = lambda c: mul12(plain12(c), plain12(c))
    elif name == "C12_CONJ_MUL":
        cases = operand_pairs(337, 2, 4)                    # the conjugate (below 3 p) enters as the first operand
        ref = lambda c: mul12(conj12(plain12(c[:12])), plain12(c[12:]))
    else:
        cases = operand_pairs(347, 4, 4)
        ref = lambda c: mul12(plain12(c[:12]), plain12(c[12:]))
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        assert_rows(o, ref(c), 2, name)
    return len(cases)


def check_line(lib, name):
    """f (L0 + L2 w^2 + L3 w^3): f below 4 p, L0 below 64 p, L2 and L3 below 2 p"""
    L = Lift(349)
    rng = L.rng
    r2 = lambda: (rng.field(P), rng.field(P))
    line = lambda l, m0=None: [L.comp(l[0][0], 64, m0), L.comp(l[0][1], 64, m0), L.comp(l[1][0], 2), L.comp(l[1][1], 2), L.comp(l[2][0], 2), L.comp(l[2][1], 2)]
    cases = []
    lines = [(ONE2, ZERO2, ZERO2), (ZERO2, ONE2, ZERO2), (ZERO2, ZERO2, ONE2), (ZERO2, ZERO2, ZERO2), ((0, 1), ZERO2, ZERO2), (ZERO2, (0, 1), ZERO2),
             (ZERO2, ZERO2, (0, 1))] + [(r2(), r2(), r2()) for _ in range(3)]
    for i, (what, f) in enumerate(structured(rng)):
        for l in (lines[i % 7], lines[7 + i % 3]):
            cases.append(L.elem(f, 4) + line(l))
    for i, (what, f) in enumerate(structured(rng)[::3]):
        cases.append(L.elem(f, 4, 3) + line(lines[7 + i % 3], 63))
    edge_line = lambda: [L.edge(64), L.edge(64), L.edge(2), L.edge(2), L.edge(2), L.edge(2)]
    for _ in range(24):
        cases.append(L.edges(4) + edge_line())
    for row in range(12):
        cases.append(L.one_edge(4, row) + edge_line())
        cases.append(L.one_edge(4, row) + L.small(6))
    for s in range(6):
        cases.append(L.small() + L.one_edge(64 if s < 2 else 2, s, 6))
        cases.append(L.edges(4) + L.one_edge(64 if s < 2 else 2, s, 6))
    cases += [L.runs() + L.runs(6) for _ in range(6)]
    for c in cases:
        bounded(c[:12], 4)
        bounded(c[12:14], 64)
        bounded(c[14:], 2)
    limb_forms_present(cases)
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        l = [val(s) * RINV % P for s in c[12:]]
        g = ((l[0], l[1]), ZERO2, (l[2], l[3]), (l[4], l[5]), ZERO2, ZERO2)
        assert_rows(o, mul12(plain12(c[:12]), g), 2, name)
    return len(cases)


def check_cyc_sqr(lib, name):
    """z^2 for z in the cyclotomic subgroup, every component lifted to the representatives below 4 p"""
    frobenius_is_validated()
    L = Lift(353)
    els = cyclotomic(40)
    cases = []
    for i, z in enumerate(els):
        cases.append(L.elem(z, 4))
        cases.append(L.elem(z, 4, 3 if i % 2 else 0))
    for i in range(12):                                      # one row in the top representative, the rest in the lowest
        s = L.elem(els[1 + i % 6], 4, 0)
        s[i] = L.comp(els[1 + i % 6][i // 2][i % 2], 4, 3)
        cases.append(s)
    for i in range(12):
        s = L.elem(els[1 + i % 6], 4, 3)
        s[i] = L.comp(els[1 + i % 6][i // 2][i % 2], 4, 0)
        cases.append(s)
    for c in cases:
        bounded(c, 4)
        z = plain12(c)
        assert mul12(z, conj12(z)) == ONE12 and mul12(frob12(frob12(z, 2), 2), z) == frob12(z, 2)        # z^(q^4 - q^2 + 1) = 1
    assert any(val(s) >= 3 * P for c in cases for s in c)
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        z = plain12(c)
        assert_rows(o, mul12(z, z), 2, name)
    return len(cases)


def check_mul_fq2(lib, name):
    """row (k, c): component c of conj^j(a_k) g, with the row's own g = g0 + g1 u (below 2 p); a below 4 p"""
    j = int(name[-1])
    frobenius_is_validated()
    L = Lift(359 + j)
    rng = L.rng
    r2 = lambda: (rng.field(P), rng.field(P))
    cases, kinds = [], []

    def case(a_slots, gs, kind):
        cases.append(a_slots + gs)
        kinds.append(kind)

    st = structured(rng)
    same = lambda g, m=None: [L.comp(g[e], 2, m) for _ in range(12) for e in range(2)]
    frob_g = lambda m=None: [L.comp(gamma(j, r // 2)[e], 2, m) for r in range(12) for e in range(2)]
    for i, (what, a) in enumerate(st):
        case(L.elem(a, 4), frob_g(), "frob")                                 # the Frobenius map (j = 0: the identity)
        case(L.elem(a, 4), same(r2()), "scale")                              # the scaling by one Fq2 value
        case(L.elem(a, 4), [L.comp(rng.field(P), 2) for _ in range(24)], "rows")   # every row its own g
    for i, (what, a) in enumerate(st[::4]):
        case(L.elem(a, 4, 3), frob_g(1), "frob")
    for _ in range(20):
        case(L.edges(4), L.edges(2, 24), "rows")
    for row in range(12):
        case(L.one_edge(4, row), L.small(24), "rows")
        case(L.small(), L.one_edge(2, 2 * row, 24), "rows")
        case(L.edges(4), L.one_edge(2, 2 * row + 1, 24), "rows")
    for _ in range(6):
        case(L.runs(), L.runs(24), "rows")
    case(L.elem(ZERO12, 4), same(ZERO2), "scale")
    case(L.elem(ONE12, 4), same(ONE2), "scale")
    for c in cases:
        bounded(c[:12], 4)
        bounded(c[12:], 2)
    limb_forms_present(cases)
    out = run(lib, name, cases)
    for c, o, kind in zip(cases, out, kinds):
        a = plain12(c[:12])
        g = [val(s) * RINV % P for s in c[12:]]
        rows = [mul2(conj2j(a[r // 2], j), (g[2 * r], g[2 * r + 1]))[r % 2] for r in range(12)]
        want = tuple((rows[2 * k], rows[2 * k + 1]) for k in range(6))
        if kind == "frob":
            assert want == frob12(a, j)
        elif kind == "scale":
            assert want == mul12(tuple(conj2j(x, j) for x in a), ((g[0], g[1]),) + (ZERO2,) * 5)
        assert_rows(o, want, 2, (name, kind))
    return len(cases)


def check_conj(lib, name):
    """a^(q^6) of an element below 2 p: below 3 p"""
    L = Lift(367)
    rng = L.rng
    cases = [L.elem(a, 2) for _, a in structured(rng)] + [L.elem(a, 2, 1) for _, a in structured(rng)]
    cases += [L.edges(2) for _ in range(24)] + [L.one_edge(2, row) for row in range(12)] + [L.small() for _ in range(6)]
    cases += [[pick(operands(2), 13 * i + r) for r in range(12)] for i in range(30)] + [L.runs() for _ in range(6)]
    for c in cases:
        bounded(c, 2)
    limb_forms_present(cases)
    assert any(s == [0] * 14 for c in cases for s in c[2:4])    # a row of zero limbs on an odd power of w
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        got, want = plain12(o), conj12(plain12(c))
        for r in range(12):
            # 3 p - a: below 3 p, and 3 p itself only for the row whose limbs are all zero (the comment said "below 3 p")
            fc.assert_weak(o[r], (name, r))
            assert val(o[r]) < 3 * P or (val(o[r]) == 3 * P and c[r] == [0] * 14), (name, r)
            assert got[r // 2][r % 2] == want[r // 2][r % 2], (name, r)
        for r in range(0, 12, 4):                               # the rows of even powers of w come back as they are
            assert o[r] == c[r] and o[r + 1] == c[r + 1]
    return len(cases)


def check_exp_x(lib, name):
    """conj(z^|x|) for z in the cyclotomic subgroup"""
    L = Lift(373)
    els = cyclotomic(24)
    cases = [L.elem(z, 4) for z in els] + [L.elem(z, 4, 3) for z in els[:12]] + [L.elem(z, 4, 0) for z in els[12:]]
    cases += [L.elem(z, 2, 1) for z in els[:8]]               # (as the final exponentiation calls it: products, below 2 p)
    for c in cases:
        bounded(c, 4)
        z = plain12(c)
        assert mul12(z, conj12(z)) == ONE12
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        assert_rows(o, conj12(pow12(plain12(c), BLS_X)), 3, name)
    return len(cases)


def check_inv(lib, name):
    """1 / f, checked by multiplying back; f below 2 p (its conjugate is taken), the Frobenius constants below 2 p; 0 -> 0"""
    L = Lift(379)
    rng = L.rng
    frob = lambda m=None: [L.comp(gamma(j, k)[e], 2, m) for j in (1, 2) for k in range(6) for e in range(2)]
    els = [a for _, a in structured(rng)][:2] + [a for w, a in structured(rng) if w != "zero" and w != "one"][::2]
    els += [rand12(rng) for _ in range(8)] + cyclotomic(4)[1:]
    cases = [L.elem(a, 2) + frob() for a in els] + [L.elem(a, 2, 1) + frob(1) for a in els[::3]]
    cases += [L.elem(ZERO12, 2, m) + frob() for m in (0, 1)]
    cases = cases[:64]
    assert any(plain12(c[:12]) == ZERO12 for c in cases)
    assert any(plain12(c[:12])[1:] == (ZERO2,) * 5 and plain12(c[:12])[0] != ONE2 and plain12(c[:12]) != ZERO12 for c in cases)      # in Fq2
    assert any(all(x == ZERO2 for x in plain12(c[:12])[1::2]) and plain12(c[:12])[2] != ZERO2 for c in cases)                      # in Fq6
    for c in cases:
        bounded(c, 2)
    out = run(lib, name, cases)
    for c, o in zip(cases, out):
        f = plain12(c[:12])
        got = plain12(o)
        for r in range(12):
            fc.assert_weak(o[r], (name, r))
            assert val(o[r]) < 2 * P, (name, r)
        assert mul12(got, f) == (ZERO12 if f == ZERO12 else ONE12), name
        if f == ZERO12:
            assert got == ZERO12
    return len(cases)


def check_export(lib, name):
    """the canonical Montgomery words (radix 2^384) of the twelve components in the F12 order of pairing.h: c0.c0 c0.c1 c0.c2
    c1.c0 c1.c1 c1.c2, 24 words each (c0 then c1); the tower's c0.cj is the coefficient of w^(2 j), c1.cj that of w^(2 j + 1)"""
    L = Lift(383)
    rng = L.rng
    cases = [L.elem(a, 4) for _, a in structured(rng)] + [L.edges(4) for _ in range(30)] + [L.one_edge(4, row) for row in range(12)]
    cases += [[pick(operands(4), 17 * i + r) for r in range(12)] for i in range(40)] + [L.runs() for _ in range(6)]
    for c in cases:
        bounded(c, 4)
    limb_forms_present(cases)
    out = run(lib, name, cases)
    inv256 = pow(256, -1, P)
    tower = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]                  # (c_i, c_j) in the order of the words
    for c, o in zip(cases, out):
        assert len(o) == 144
        for t, (i, j) in enumerate(tower):
            k = 2 * j + i
            for e in range(2):
                got = sum(w << (32 * x) for x, w in enumerate(o[t * 24 + 12 * e:t * 24 + 12 * e + 12]))
                assert got == val(c[2 * k + e]) * inv256 % P, (name, k, e)
    return len(cases)


def checker(name):
    if name in ("C12_MUL", "C12_SQR", "C12_CONJ_MUL"):
        return check_mul
    if name.startswith("C12_MUL_FQ2_J"):
        return check_mul_fq2
    return {"C12_LINE": check_line, "C12_CYC_SQR": check_cyc_sqr, "C12_CONJ": check_conj, "C12_EXP_X": check_exp_x, "C12_INV": check_inv,
            "C12_EXPORT": check_export}[name]


def check_op(lib, name):
    """One hook call for the op; returns the number of cases it sent."""
    return checker(name)(lib, name)


def reference_agrees_with_the_oracle():
    """mul12 (schoolbook, written here) against oracle/pairing.py fq12_mul / tower_to_w, once"""
    rng = synth.SplitMix64(389)
    for _ in range(8):
        a, b = rand12(rng), rand12(rng)
        assert opair.fq12_mul(a, b) == mul12(a, b)
        assert opair.fq12_conj(a) == conj12(a)
    assert opair.tower_to_w(((1, 2), (3, 4), (5, 6)), ((7, 8), (9, 10), (11, 12))) == ((1, 2), (7, 8), (3, 4), (9, 10), (5, 6), (11, 12))
    w = tuple(ONE2 if k == 1 else ZERO2 for k in range(6))
    assert pow12(w, 6) == (XI,) + (ZERO2,) * 5


def op_table_and_the_first_code_past_it(lib):
    """The ops of the C source are OPS in their order; the last code is taken and the first one past it refused without
    touching the output."""
    assert ops_of_the_c_source() == OPS
    fn = lib.dll.zk_hook_c12_op
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    a = np.zeros((1, 36, 16), dtype=np.uint32)
    out = np.full((1, 192), 7, dtype=np.uint32)
    assert fn(len(OPS) - 1, 0, a.ctypes.data, out.ctypes.data) == 0
    assert fn(len(OPS), 1, a.ctypes.data, out.ctypes.data) == fc.ZK_ERR_INVALID_ARGUMENT
    assert (out == 7).all()
