"""Cases for the device field arithmetic and the XYZZ group law, shared by the emulation (CPU) and the GPU tests of
tests/test_field_ops.py.  Every op of the test hook zk_hook_field_op (csrc/field_hooks.cpp) gets rows of operands whose
limbs the case builder chooses one by one, and every output row is compared with Python integers / oracle/bls12_381.py and
with the contract the header states for it (dev_field.h, dev_curve.h).

The operands are the ones random data never produces: values k p + r for every k the operand's bound admits and r in
{0, 1, p - 1, random}; the same value with its limbs exact and with every limb raised to 2^28 + 8 that the value allows;
the pattern [2^28 + 8] * 13 + [top]; un-normalised operands as sub_raw leaves them; products just under the limits the
routines are checked for; operands that make a product land on 0 or on p.  A builder asserts the preconditions of its op
(the inequalities of the ZK_FQ28_CHECK lines) on every row before it is sent."""
import ctypes as C
import functools
import os
import re
from fractions import Fraction

import numpy as np

from oracle import bls12_381 as bls
from oracle import synth

P = bls.Q_MOD
W = 1 << 28
MASK = W - 1
WK = W + 8                      # the largest weakly normalised limb
R392 = pow(2, 392, P)           # the Montgomery radix of Fq28
RINV = pow(R392, -1, P)
P13 = P >> 364                  # top limb of p
MO, BX, BY = 2, 10, 5           # dev_curve.h: a product < MO p, a stored X < BX p, Y < BY p
BS = (2, 4, 5, 7, 10, 15, 63)   # MO, 2 MO, BY, 3 MO + 1, BX, FQ2_SPREAD_K - 1, the last spread constant
SQR_AS = (2, 4, 5, 6, 8, 10, 13, 30)
ZK_ERR_INVALID_ARGUMENT = 16   # include/zkamd.h
# The emulation build evaluates the ZK_FQ28_CHECK inequalities in long double, where (B p - 1) / p rounds to B: every row
# stays 2^-40 (relative) inside each limit, so that the checker's rounding cannot abort on an admissible row.
MARGIN = Fraction(1, 1 << 40)
EPS = P >> 39


def _op_table():
    t = [("FQ28_ADD", 2, 1), ("FQ28_DBL", 1, 1)]
    for b in BS:
        t += [("FQ28_SUB_B_%d" % b, 2, 1), ("FQ28_NEG_B_%d" % b, 1, 1), ("FQ28_SUB_RAW_%d" % b, 2, 1), ("FQ28_NEG_RAW_%d" % b, 1, 1),
              ("FQ2X_SUB_B_%d" % b, 4, 2)]
    t += [("FQ28_SUB_SUB2_2_2", 3, 1), ("FQ28_MUL", 2, 1), ("FQ28_SQR", 1, 1), ("FQ28_MUL_RAW_10", 3, 1), ("FQ28_MUL_SUB2_2", 4, 1),
          ("FQ28_MUL_SUB2_5", 4, 1), ("FQ28_CANON", 1, 1), ("FQ28_WRED", 1, 1), ("FQ28_IS_ZERO_FULL", 1, 1), ("FQ28_IS_ZERO_LAZY", 1, 1),
          ("FQ28_UNPACK", 1, 1), ("FQ28_IMPORT", 1, 1), ("FQ28_EXPORT", 1, 1), ("FQ2X_ADD", 4, 2), ("FQ2X_SUB_SUB2_2_2", 6, 2),
          ("FQ2X_MUL", 4, 2)]
    t += [("FQ2X_SQR_B_%d" % a, 2, 2) for a in SQR_AS]
    t += [("FQ2X_IS_ZERO_FULL", 2, 1)]
    for f in ("FR", "FQ32"):
        t += [(f + "_ADD", 2, 1), (f + "_SUB", 2, 1), (f + "_NEG", 1, 1), (f + "_DBL", 1, 1), (f + "_SQR", 1, 1), (f + "_TO_MONT", 1, 1),
              (f + "_FROM_MONT", 1, 1)]
    for g, w in (("G1", 1), ("G2", 2)):
        t += [(g + "_MDBL", 2 * w, 4 * w), (g + "_XDBL", 4 * w, 4 * w), (g + "_MADD", 6 * w, 4 * w), (g + "_MADD_NEG", 6 * w, 4 * w),
              (g + "_XADD", 8 * w, 4 * w)]
    return t


OPS = _op_table()               # the order of enum FieldOp in csrc/field_hooks.cpp
OP_NAMES = [n for n, _, _ in OPS]
OP_CODE = {n: i for i, n in enumerate(OP_NAMES)}


def ops_of_the_c_source(table="ZK_HK_OPS"):
    """The names of enum FieldOp (table ZK_HK_OPS) or of the row ops that continue its codes (ZK_HK_COOP_OPS) as the
    preprocessor would list them, read from csrc/field_hooks.cpp."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zero-chain_amd", "csrc", "field_hooks.cpp")).read()
    src = src.replace("\\\n", " ")
    macros = {m.group(1): m.group(2) for m in re.finditer(r"^#define (ZK_HK_\w+)\(X[^)]*\)\s+(.*)$", src, flags=re.M)}

    def expand(body, args):
        names = []
        for m in re.finditer(r"\b(X|ZK_HK_B|ZK_HK_FP|ZK_HK_GROUP|ZK_HK_CB|ZK_HK_CGROUP)\(X?,?\s*([^,)]+)", body):
            kind, first = m.group(1), m.group(2).strip()
            if kind == "X":
                for k, v in args.items():
                    first = first.replace(k + "##", v).replace("##" + k, v)
                names.append(first.replace("##", ""))
            else:
                names += expand(macros[kind], {"B": first} if kind in ("ZK_HK_B", "ZK_HK_CB") else {"P": first})
        return names
    return expand(macros[table], {})


# ------------------------------------------------------------------------------------------------ limbs
def val(l):
    return sum(int(x) << (28 * i) for i, x in enumerate(l))


def exact(v):
    l = [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]
    assert 0 <= v and l[13] < (1 << 32)
    return l


def weak(v):
    """The limbs of v with every limb raised by 2^28 that the value allows: a limb <= 8 borrows from the limbs above it."""
    l = exact(v)
    for i in range(13):
        if l[i] <= 8 and any(l[i + 1:]):
            l[i] += W
            j = i + 1
            while l[j] == 0:
                l[j] = MASK
                j += 1
            l[j] -= 1
    assert val(l) == v and all(x <= WK for x in l[:13])
    return l


def sprinkled(v, rng):
    """v with about half of its low limbs replaced by 0 .. 8 (so that the weak form has limbs at 2^28 + 0 .. 8), weak form."""
    l = exact(v)
    for i in range(13):
        if rng.below(2):
            l[i] = 8 if rng.below(2) else rng.below(9)
    return weak(val(l))


def pattern(top):
    return [WK] * 13 + [top]


LOW_WK = val([WK] * 13)


def ratio(l):
    return Fraction(val(l), P)


def spread(m):
    """The spread form of m p (tools/gen_constants.py), recomputed here from p."""
    c = exact(m * P)
    sp = [c[0] + 3 * W] + [c[i] + 3 * W - 3 for i in range(1, 13)] + [c[13] - 3]
    assert val(sp) == m * P
    return sp


RAW_LIMB_BOUND = 2 ** 30.4      # dev_field.h: limbs of a sub_raw / neg_raw result


@functools.lru_cache(maxsize=None)
def operands(bound, seed=1, nrand=2):
    """Limb vectors of values < bound p: k p + r in both limb forms for every k, sprinkled values, the all-(2^28 + 8) pattern."""
    rng = synth.SplitMix64(1000 * seed + bound)
    out = []
    for k in range(bound):
        for r in [0, 1, P - 1] + [rng.field(P) for _ in range(nrand)]:
            v = min(k * P + r, bound * P - EPS)
            e, w = exact(v), weak(v)
            out.append(e)
            if w != e:
                out.append(w)
        s = sprinkled(k * P + rng.field(P), rng)
        if val(s) <= bound * P - EPS:
            out.append(s)
    tops = {0, (bound * P - EPS - LOW_WK) >> 364} | {k * P13 + d for k in range(1, bound) for d in (-1, 0, 1)}
    for top in sorted(tops):
        if 0 <= top and val(pattern(top)) <= bound * P - EPS:
            out.append(pattern(top))
    for l in out:
        assert val(l) <= bound * P - EPS and all(0 <= x <= WK for x in l[:13])
    return out


def pick(lst, i, mult=7, off=3):
    return lst[(i * mult + off) % len(lst)]


# ------------------------------------------------------------------------------------------------ the hook
def run(lib, name, rows):
    """rows: one list of input slots per row, a slot a list of up to 16 words.  Returns one list of output slots (14 limbs)
    per row.  The launch always ends in a partial wave."""
    code, (_, ni, no) = OP_CODE[name], OPS[OP_CODE[name]]
    return launch(lib, name, code, ni, no, rows, 64)


def launch(lib, name, code, ni, no, rows, wave):
    """One call of the hook for op `code` (ni -> no slots), `wave` rows to a GPU wave."""
    assert rows and all(len(r) == ni for r in rows), name
    rows = list(rows)
    first = len(rows)
    while len(rows) < wave + 1 or len(rows) % wave == 0:      # one full wave and a partial one at the least: repeat rows
        rows.append(rows[len(rows) % first])
    n = len(rows)
    assert n % wave != 0 and n <= 6000, (name, n)
    a = np.zeros((n, ni, 16), dtype=np.uint32)
    for i, r in enumerate(rows):
        for s, slot in enumerate(r):
            a[i, s, :len(slot)] = slot
    a[:, :, 14:] = 0xdeadbeef       # the pad words are ignored
    out = np.full((n, no, 16), 0xa5a5a5a5, dtype=np.uint32)
    fn = lib.dll.zk_hook_field_op
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.check(fn(code, a.ctypes.data, out.ctypes.data, n))
    assert not out[:, :, 14:].any(), name
    return [[[int(x) for x in out[i, s, :14]] for s in range(no)] for i in range(n)], rows


# ------------------------------------------------------------------------------------------------ output contracts
def assert_weak(l, what):
    assert all(x <= WK for x in l[:13]), (what, [hex(x) for x in l])


def assert_product(l, want_residue, what):
    """a product: exactly normalised, < 2 p, the right residue"""
    assert all(x < W for x in l[:13]), (what, [hex(x) for x in l])
    v = val(l)
    assert v < 2 * P, (what, hex(v))
    assert v % P == want_residue % P, (what, hex(v))


def mont(x):
    return x * RINV % P          # a b 2^-392


# ------------------------------------------------------------------------------------------------ Fq28 linear ops
def rows_add():
    rows = []
    for ka in range(63):
        la, lb = operands(ka + 1), operands(63 - ka)
        for i, a in enumerate(x for x in la if val(x) >= ka * P):
            rows.append([a, pick(lb, len(rows))])
        rows.append([la[-1], lb[-1]])                       # all limbs 2^28 + 8 in both
        rows.append([exact((ka + 1) * P - EPS), exact((63 - ka) * P)])   # a + b just under 64 p
    return rows


def rows_sub(b_bound, lift):
    """(a, b) with b < b_bound p and a + lift p - b < 64 p"""
    rows = []
    lb = operands(b_bound)
    la = operands(64 - lift) if lift < 64 else [exact(0)]
    stride = max(1, len(lb) * 3 // 2500)
    for i, b in enumerate(lb):
        cand = [exact(0)]
        if i % stride == 0:
            cand += [pick(la, i), pick(la, i, 13, 5), la[-1]]
        lim = (64 - lift) * P + val(b) - EPS              # the largest a: the result is just under 64 p
        if lim >= 0:
            cand += [exact(lim), weak(lim)]
        for a in cand:
            if val(a) + lift * P - val(b) <= 64 * P - EPS:
                rows.append([a, b])
    return rows


def check_fq28_linear(lib, name, run=run):
    if name == "FQ28_ADD":
        rows = rows_add()
        want = lambda r: val(r[0]) + val(r[1])
    elif name == "FQ28_DBL":
        rows = [[a] for a in operands(32)]
        want = lambda r: 2 * val(r[0])
    elif name == "FQ28_SUB_SUB2_2_2":
        rows = []
        l2 = operands(2)
        for i, a in enumerate(operands(57)):
            rows.append([a, pick(l2, i), pick(l2, i, 5, 1)])
        for b in l2:
            for c in l2:
                rows.append([exact(0), b, c])
                rows.append([pattern(0), b, c])
        rows.append([exact(57 * P - EPS), exact(0), exact(0)])
        for r in rows:
            assert ratio(r[1]) < 2 and ratio(r[2]) < 2
        want = lambda r: val(r[0]) + 7 * P - val(r[1]) - 2 * val(r[2])
    else:
        kind, b = name.rsplit("_", 1)
        b = int(b)
        if kind in ("FQ28_SUB_B", "FQ28_SUB_RAW"):
            rows = rows_sub(b, b + 1)
            want = lambda r: val(r[0]) + (b + 1) * P - val(r[1])
            for r in rows:
                assert ratio(r[1]) < b
        else:
            rows = [[x] for x in operands(b) if (b + 1) * P - val(x) <= 64 * P - EPS]      # (B = 63: 64 p - 0 is not a stored value)
            want = lambda r: (b + 1) * P - val(r[0])
    raw = "_RAW_" in name
    if raw:
        # dev_field.h: "limbs < 2^30.4", from the spread constant: a_i + V_i - b_i <= 2^28 + 8 + V_i
        v = spread(int(name.rsplit("_", 1)[1]) + 1)
        bound = [WK + v[i] for i in range(13)]
        assert max(bound) < RAW_LIMB_BOUND
    out, rows = run(lib, name, rows)
    for r, o in zip(rows, out):
        assert val(o[0]) == want(r), (name, r)
        if raw:
            assert all(o[0][i] <= bound[i] for i in range(13)), (name, r)
        else:
            assert val(o[0]) < 64 * P
            assert_weak(o[0], (name, r))
    return len(rows)


# ------------------------------------------------------------------------------------------------ Fq28 products
def raw_operand(b, top_x):
    """What sub_raw<b> leaves at its largest limbs: x = [2^28 + 8] * 13 + [top_x] minus a subtrahend whose low limbs are 0."""
    v = spread(b + 1)
    return [WK + v[i] for i in range(13)] + [top_x + v[13]]


def largest_k(limit, other):
    """the largest k <= 63 with (k + 1) * other < limit (other: an upper bound of the partner's ratio), or -1"""
    limit = Fraction(limit) - 2 * MARGIN
    k = min(63, int(limit / other) - 1) if other > 0 else 63
    while k >= 0 and (k + 1) * other >= limit:
        k -= 1
    return k


def rows_mul():
    rng = synth.SplitMix64(41)
    rows = []
    rs = lambda: [0, 1, P - 1, rng.field(P)]
    for ka in range(64):
        for kb in sorted({0, 1, largest_k(2500, ka + 1), rng.below(largest_k(2500, ka + 1) + 1)}):
            for i, (ra, rb) in enumerate(zip(rs(), reversed(rs()))):
                a, b = ka * P + ra, kb * P + rb
                s = sprinkled(b, rng)
                rows.append([exact(a), exact(b)] if i % 2 else [weak(a), s if val(s) < (kb + 1) * P else exact(b)])
        rows.append([exact(ka * P), exact(largest_k(2500, ka + 1) * P)])           # multiples of p: the product is 0 or p
    rows.append([exact(49 * P), exact(50 * P)])
    rows.append([exact(49 * P + 5), exact(49 * P + 5)])
    rows.append([exact(50 * P - EPS), exact(50 * P - EPS)])
    # all limbs 2^28 + 8 in both operands, at every top the 2500 p^2 limit admits
    for ka in range(1, 64):
        ta = ka * P13
        tb = largest_k(2500, Fraction(val(pattern(ta)), P) + Fraction(1, 1000)) * P13
        rows.append([pattern(ta), pattern(max(tb, 0))])
    rows.append([pattern(0), pattern(0)])
    # a raw FIRST operand (sub_raw / neg_raw at their largest limbs) against weak and exact second operands
    for b in BS[:-1]:
        for top_x in (0, P13, (61 - b) * P13):
            a = raw_operand(b, top_x)
            assert ratio(a) < 64
            kb = largest_k(2500, ratio(a))
            for second in (pattern(max(0, (kb + 1) * P13 - P13 - 2)), exact(kb * P + P - 1), exact(P), exact(0)):
                if ratio(a) * ratio(second) <= 2500 - MARGIN:
                    rows.append([a, second])
    for r in rows:
        assert ratio(r[0]) * ratio(r[1]) <= 2500 - MARGIN and ratio(r[0]) < 64 and ratio(r[1]) < 64
        assert all(x <= WK for x in r[1][:13]) and all(x < RAW_LIMB_BOUND for x in r[0][:13])
    return rows


def check_fq28_mul(lib, name, run=run, assert_product=assert_product):
    if name == "FQ28_MUL":
        rows = rows_mul()
        want = lambda r: mont(val(r[0]) * val(r[1]))
    elif name == "FQ28_SQR":
        rows = [[a] for a in operands(50)] + [[exact(49 * P + 5)], [exact(50 * P - EPS)]]
        for r in rows:
            assert ratio(r[0]) ** 2 <= 2500 - MARGIN
        want = lambda r: mont(val(r[0]) ** 2)
    else:   # FQ28_MUL_RAW_10: mul(sub_raw<10>(x, y), c)
        rows = []
        rng = synth.SplitMix64(43)
        l10, l2 = operands(10), operands(2)
        for i, y in enumerate(l10):
            for x in (pick(l2, i), pattern(P13), exact(0)):
                a = val(x) + 11 * P - val(y)
                kc = largest_k(2500, Fraction(a, P))
                for c in (pattern(max(0, kc * P13 - 2)), exact(kc * P + rng.field(P)), pick(operands(13), i)):
                    if Fraction(a, P) * ratio(c) <= 2500 - MARGIN:
                        rows.append([x, y, c])
        for r in rows:
            assert ratio(r[1]) < 10
        want = lambda r: mont((val(r[0]) + 11 * P - val(r[1])) * val(r[2]))
    out, rows = run(lib, name, rows)
    for r, o in zip(rows, out):
        assert_product(o[0], want(r), (name, r))
    return len(rows)


def rows_mul_sub2(b):
    """(x0, y0, x1, y1): x1 < b p, |x0||y0| + (b + 1)|y1| < 2000"""
    rng = synth.SplitMix64(47 + b)
    rows = []
    lx1 = operands(b)
    for i, x1 in enumerate(lx1):
        for k1 in sorted({0, 1, 63, rng.below(64)}):
            y1 = pick(operands(k1 + 1), i + k1, 11, len(operands(k1 + 1)) - 1 - (i % 5))
            budget = 2000 - (b + 1) * ratio(y1)
            k0 = (0, 1, 12, 44, 63)[i % 5]
            ky = largest_k(budget, k0 + 1)
            if ky < 0:
                continue
            x0 = pick(operands(k0 + 1), i, 3, len(operands(k0 + 1)) - 1)
            for y0 in (exact(ky * P + P - 1), pattern(max(0, ky * P13 - 1)) if ky else exact(1), exact(ky * P)):
                rows.append([x0, y0, x1, y1])
        # x0 y0 = x1 y1 mod p under other representatives: the difference is a multiple of p
        y = pick(operands(13), i)
        x0 = exact(val(x1) % P + P) if i % 2 else exact(val(x1) % P)
        rows.append([x0, y, x1, y])
        rows.append([y, x0, x1, y])
    # a raw y0 (t = sub_raw<BX>(q, x3) of madd / xadd) next to a weakly normalised x0, at the largest limbs
    for top_x in (0, P13):
        y0 = raw_operand(BX, top_x)
        for x1 in (lx1[-1], exact(b * P - EPS), exact(0)):
            for y1 in (pattern(P13), exact(2 * P - 1), exact(0)):
                budget = 2000 - (b + 1) * ratio(y1)
                k0 = largest_k(budget, ratio(y0))
                for x0 in (pattern(max(0, k0 * P13 - 2)), exact(k0 * P + P - 1)):
                    if ratio(x0) * ratio(y0) <= budget - MARGIN:
                        rows.append([x0, y0, x1, y1])
    for r in rows:
        assert ratio(r[2]) <= b - MARGIN and ratio(r[0]) * ratio(r[1]) + (b + 1) * ratio(r[3]) <= 2000 - MARGIN
        assert all(x <= WK for s in (r[0], r[2], r[3]) for x in s[:13]) and all(x < RAW_LIMB_BOUND for x in r[1][:13])
    return rows


def check_fq28_mul_sub2(lib, name, run=run, assert_product=assert_product):
    b = int(name.rsplit("_", 1)[1])
    out, rows = run(lib, name, rows_mul_sub2(b))
    for r, o in zip(rows, out):
        assert_product(o[0], mont(val(r[0]) * val(r[1]) - val(r[2]) * val(r[3])), (name, r))
    return len(rows)


# ------------------------------------------------------------------------------------------------ reductions, zero tests
def rows_wred():
    rng = synth.SplitMix64(53)
    rows = [[a] for a in operands(64)]
    for k in range(64):
        for base in (k * P13, k * (P13 + 1)):
            for d in range(-4, 5):
                top = base + d
                if top < 0:
                    continue
                for low in ([0] * 13, [WK] * 13, [rng.below(W) for _ in range(13)]):
                    if val(low + [top]) <= 64 * P - EPS:
                        rows.append([low + [top]])
    return rows


def rows_zero():
    rows = [[exact(k * P)] for k in range(64)] + [[weak(k * P)] for k in range(64)]
    rows += [[exact(k * P + d)] for k in range(64) for d in (1, P - 1, 1 << 364, 1 << 28)]
    rows += [[a] for a in operands(64)[::3]]
    return rows


def check_fq28_unary(lib, name, run=run):
    if name == "FQ28_CANON":
        out, rows = run(lib, name, [[a] for a in operands(64)])
        for r, o in zip(rows, out):
            assert o[0] == exact(val(r[0]) % P), (name, r)
    elif name == "FQ28_WRED":
        out, rows = run(lib, name, rows_wred())
        for r, o in zip(rows, out):
            v = val(o[0])
            assert all(x < W for x in o[0][:13]) and o[0][13] < (1 << 31), (name, r, o)
            assert v % P == val(r[0]) % P and v < 3 * P, (name, r, o)
    else:
        out, rows = run(lib, name, rows_zero())
        for r, o in zip(rows, out):
            assert o[0] == [int(val(r[0]) % P == 0)] + [0] * 13, (name, r)
        assert sum(o[0][0] for o in out) >= 64
    return len(rows)


def host_values():
    rng = synth.SplitMix64(59)
    vs = [0, 1, P - 1, P - 2, bls.FQ_R, (1 << 384) - 1 - P * (((1 << 384) - 1) // P)]
    vs += [((1 << (32 * k)) + d) % P for k in range(1, 12) for d in (-1, 0, 1)] + [P - (1 << (32 * k)) for k in range(1, 12)]
    vs += [((1 << (28 * k)) + d) % P for k in range(1, 14) for d in (-1, 0, 1)]
    vs += [rng.field(P) for _ in range(100)]
    return vs


def words32(v, n=12):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def check_fq28_host(lib, name, run=run, assert_product=assert_product):
    if name == "FQ28_UNPACK":
        vs = host_values() + [(1 << 384) - 1, (1 << 384) - (1 << 32), 1 << 383]
        out, rows = run(lib, name, [[words32(v)] for v in vs])
        for r, o in zip(rows, out):
            assert o[0] == exact(sum(w << (32 * i) for i, w in enumerate(r[0]))), (name, r)
    elif name == "FQ28_IMPORT":
        # x 2^384 (the host's Montgomery form) -> x 2^392: the product with KIN = 2^400
        out, rows = run(lib, name, [[words32(v)] for v in host_values()])
        for r, o in zip(rows, out):
            m = sum(w << (32 * i) for i, w in enumerate(r[0]))
            assert_product(o[0], m * 256, (name, r))
    else:
        # x 2^392 -> x 2^384, canonical: the product with KOUT = 2^384
        out, rows = run(lib, name, [[a] for a in operands(64)])
        inv256 = pow(256, -1, P)
        for r, o in zip(rows, out):
            got = sum(w << (32 * i) for i, w in enumerate(o[0][:12]))
            assert o[0][12:] == [0, 0] and all(w < (1 << 32) for w in o[0])
            assert got == val(r[0]) * inv256 % P, (name, r)
    return len(rows)


# ------------------------------------------------------------------------------------------------ Fq2x
def pair_rows(rows):
    """Rows of an Fq28 op -> rows of the component-wise Fq2x op: c0 from one row, c1 from another."""
    n = len(rows)
    out = []
    for i in range(n):
        r0, r1 = rows[i], rows[(i * 5 + 3) % n]
        out.append([s for pair in zip(r0, r1) for s in pair])
    return out


def check_fq2x_linear(lib, name, run=run):
    if name == "FQ2X_ADD":
        base = rows_add()
        want = lambda r: val(r[0]) + val(r[1])
    elif name == "FQ2X_SUB_SUB2_2_2":
        l2 = operands(2)
        base = [[a, pick(l2, i), pick(l2, i, 5, 1)] for i, a in enumerate(operands(57))] + [[exact(0), b, c] for b in l2 for c in l2]
        want = lambda r: val(r[0]) + 7 * P - val(r[1]) - 2 * val(r[2])
    else:
        b = int(name.rsplit("_", 1)[1])
        base = rows_sub(b, b + 1)
        want = lambda r: val(r[0]) + (b + 1) * P - val(r[1])
    out, rows = run(lib, name, pair_rows(base))
    for r, o in zip(rows, out):
        for c in (0, 1):
            got = o[c]
            assert val(got) == want(r[c::2]), (name, c, r)
            assert val(got) < 64 * P
            assert_weak(got, (name, r))
    return len(rows)


def rows_fq2x_mul():
    rng = synth.SplitMix64(61)
    rows = []
    form = lambda v, i: exact(v) if i % 2 else weak(v)
    i = 0
    top = lambda k, r, bound: min(k * P + r, bound * P - EPS)
    for k_a1 in range(15):
        for k_b1 in (0, 1, 5, 20, 63, rng.below(64)):
            for k_a0 in (0, 1, 7, 30, 63, rng.below(64)):
                k_b0 = largest_k(2000 - 16 * (k_b1 + 1), k_a0 + 1)
                while k_b0 >= 0 and (k_a0 + 1) * (k_b1 + 1) + (k_a1 + 1) * (k_b0 + 1) >= 2000:
                    k_b0 -= 1
                if k_b0 < 0:
                    continue
                for rs in ((P - 1, P - 1, P - 1, P - 1), (0, 0, 0, 0), (rng.field(P), 1, rng.field(P), 0)):
                    i += 1
                    rows.append([form(top(k_a0, rs[0], 64), i), form(top(k_a1, rs[1], 15), i + 1), form(top(k_b0, rs[2], 64), i), form(top(k_b1, rs[3], 64), i + 1)])
    # all limbs 2^28 + 8: a1 at the 15 p the routine's internal negation allows
    top15 = (15 * P - EPS - LOW_WK) >> 364
    for ta0, tb0, tb1 in ((0, 0, 0), (P13, 2 * P13, P13), (12 * P13, 12 * P13, 12 * P13), (30 * P13, 20 * P13, 40 * P13)):
        rows.append([pattern(ta0), pattern(top15), pattern(tb0), pattern(tb1)])
    for r in rows:
        a0, a1, b0, b1 = (ratio(x) for x in r)
        assert a1 <= 15 - MARGIN and a0 * b0 + 16 * b1 <= 2000 - MARGIN and a0 * b1 + a1 * b0 <= 2000 - MARGIN
    return rows


def rows_fq2x_sqr(a_bound):
    rng = synth.SplitMix64(67 + a_bound)
    rows = []
    i = 0
    for k1 in range(a_bound):
        for k0 in sorted({0, 1, 2, 5, 9, 12, 20, 30, min(k1, 30), max(k1 - 1, 0), min(k1 + 1, 30)}):
            # upper bounds of the operands of the two products: s = a0 + a1, d = a0 + (A + 1) p - a1, t = 2 a0
            if (k0 + k1 + 2) * (k0 + 1 + a_bound + 1 - k1) >= 2500 or 2 * (k0 + 1) * (k1 + 1) >= 2500 or k0 + 1 + a_bound + 1 - k1 > 63 or k0 + k1 + 2 > 63:
                continue
            for r0, r1 in ((0, 0), (P - 1, P - 1), (1, P - 1), (rng.field(P), rng.field(P)), (0, rng.field(P))):
                i += 1
                a0, a1 = k0 * P + r0, min(k1 * P + r1, a_bound * P - EPS)
                rows.append([exact(a0), exact(a1)] if i % 2 else [weak(a0), weak(a1)])
            if k0 == k1:
                rows.append([exact(k1 * P + 5), exact(k1 * P + 5)])   # a0 = a1: the real part is a multiple of p
    rows.append([pattern(0), pattern(0)])
    rows.append([pattern(P13), pattern(max(0, (a_bound - 1) * P13 - 1))])
    for r in rows:
        a0, a1 = ratio(r[0]), ratio(r[1])
        assert a1 <= a_bound - MARGIN and (a0 + a1) * (a0 + a_bound + 1 - a1) <= 2500 - MARGIN and 2 * a0 * a1 <= 2500 - MARGIN
        assert a0 + a1 <= 64 - MARGIN and 2 * a0 <= 64 - MARGIN and a0 + a_bound + 1 - a1 <= 64 - MARGIN
    return rows


def check_fq2x_products(lib, name, run=run, assert_product=assert_product):
    if name == "FQ2X_MUL":
        out, rows = run(lib, name, rows_fq2x_mul())
        for r, o in zip(rows, out):
            a0, a1, b0, b1 = (val(x) for x in r)
            assert_product(o[0], mont(a0 * b0 - a1 * b1), (name, 0, r))
            assert_product(o[1], mont(a0 * b1 + a1 * b0), (name, 1, r))
    elif name == "FQ2X_IS_ZERO_FULL":
        z = rows_zero()
        rows = [[z[i][0], z[(i * 3 + 1) % len(z)][0]] for i in range(len(z))] + [[exact(k * P), weak((63 - k) * P)] for k in range(64)]
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            assert o[0] == [int(val(r[0]) % P == 0 and val(r[1]) % P == 0)] + [0] * 13, (name, r)
        assert sum(o[0][0] for o in out) >= 64
    else:
        out, rows = run(lib, name, rows_fq2x_sqr(int(name.rsplit("_", 1)[1])))
        for r, o in zip(rows, out):
            a0, a1 = val(r[0]), val(r[1])
            assert_product(o[0], mont((a0 + a1) * (a0 - a1)), (name, 0, r))
            assert_product(o[1], mont(2 * a0 * a1), (name, 1, r))
    return len(rows)


# ------------------------------------------------------------------------------------------------ saturated fields
def fp_values(mod, n32, seed):
    rng = synth.SplitMix64(seed)
    ones = ((1 << (32 * n32)) - 1) % mod
    vs = [0, 1, 2, mod - 1, mod - 2, ones, (mod + 1) // 2, (mod - 1) // 2]
    vs += [((1 << (32 * k)) + d) % mod for k in range(1, n32 + 1) for d in (-1, 0, 1)] + [mod - (1 << (32 * k)) % mod for k in range(1, n32)]
    vs += [rng.field(mod) for _ in range(60)]
    return vs


def check_fp(lib, name):
    f, op = name.split("_", 1)
    mod, n32 = (bls.R_MOD, 8) if f == "FR" else (P, 12)
    R = (1 << (32 * n32)) % mod
    Ri = pow(R, -1, mod)
    vs = fp_values(mod, n32, 71 + n32)
    if op in ("ADD", "SUB"):
        pairs = [(a, pick(vs, i)) for i, a in enumerate(vs)] + [(a, a) for a in vs] + [(a, (mod - a) % mod) for a in vs]
        pairs += [(a, b) for a in vs[:8] for b in vs[:8]]
        rows = [[words32(a, n32), words32(b, n32)] for a, b in pairs]
        want = (lambda a, b: (a + b) % mod) if op == "ADD" else (lambda a, b: (a - b) % mod)
    else:
        rows = [[words32(a, n32)] for a in vs]
        want = {"NEG": lambda a: (-a) % mod, "DBL": lambda a: 2 * a % mod, "SQR": lambda a: a * a * Ri % mod,
                "TO_MONT": lambda a: a * R % mod, "FROM_MONT": lambda a: a * Ri % mod}[op]
    out, rows = run(lib, name, rows)
    for r, o in zip(rows, out):
        got = sum(w << (32 * i) for i, w in enumerate(o[0][:n32]))
        args = [sum(w << (32 * i) for i, w in enumerate(s)) for s in r]
        assert not any(o[0][n32:]) and got < mod and got == want(*args), (name, [hex(x) for x in args], hex(got))
    return len(rows)


# ------------------------------------------------------------------------------------------------ the group law
class _Field:
    """Coordinates of G1 (w = 1 slot) or G2 (w = 2 slots): plain oracle elements <-> lists of slots in Montgomery form."""

    def __init__(self, g2):
        self.w = 2 if g2 else 1
        self.curve = bls.G2 if g2 else bls.G1
        self.F = self.curve.F

    def comps(self, x):
        return list(x) if self.w == 2 else [x]

    def lifted(self, x, ks, forms):
        """plain x -> slots of x 2^392 mod p + k p, one k and one limb form per component"""
        return [(weak if f else exact)(c * R392 % P + k * P) for c, k, f in zip(self.comps(x), ks, forms)]

    def plain(self, slots):
        c = [val(s) * RINV % P for s in slots]
        return tuple(c) if self.w == 2 else c[0]

    def is_zero(self, slots):
        return all(val(s) % P == 0 for s in slots)


def _points(fld, seed):
    rng = synth.SplitMix64(seed)
    c = fld.curve
    ks = [1, 2, 3, 5, rng.field(bls.R_MOD), rng.field(bls.R_MOD)]
    return [c.to_affine(c.mul(c.gen, k)) for k in ks]


class _Builder:
    def __init__(self, fld, seed):
        self.f, self.rng, self.i = fld, synth.SplitMix64(seed), 0

    def ks(self, bound):
        """the lift of each component: cycles through 0 .. bound - 1, the top of the range first"""
        self.i += 1
        return [(bound - 1 - (self.i + 3 * c)) % bound for c in range(self.f.w)]

    def forms(self):
        return [(self.i + c) % 2 for c in range(self.f.w)]

    def z(self):
        F = self.f.F
        while True:
            z = tuple(self.rng.field(P) for _ in range(2)) if self.f.w == 2 else self.rng.field(P)
            if not F.is_zero(z) and not F.eq(z, F.one):
                return z

    def xyzz(self, pt, kx=None, ky=None):
        """(x z^2, y z^3, z^2, z^3) for a random z != 1, X and Y lifted by k p below BX p and BY p, ZZ and ZZZ in [0, 2 p)"""
        F, f = self.f.F, self.f
        z = self.z()
        zz = F.sqr(z)
        zzz = F.mul(zz, z)
        kx = self.ks(BX) if kx is None else [kx] * f.w
        ky = self.ks(BY) if ky is None else [ky] * f.w
        fm = self.forms()
        return (f.lifted(F.mul(pt[0], zz), kx, fm) + f.lifted(F.mul(pt[1], zzz), ky, fm[::-1]) +
                f.lifted(zz, self.ks(MO), [0] * f.w) + f.lifted(zzz, self.ks(MO), [0] * f.w))

    def infinity(self):
        """ZZ = 0 or p, the other coordinates anything inside their bounds"""
        f = self.f
        g = lambda: tuple(self.rng.field(P) for _ in range(2)) if f.w == 2 else self.rng.field(P)
        self.i += 1
        zz = [[exact(0)] * f.w, [exact(P)] * f.w, [exact(P * ((self.i + c) % 2)) for c in range(f.w)]][self.i % 3]
        return f.lifted(g(), self.ks(BX), self.forms()) + f.lifted(g(), self.ks(BY), self.forms()) + zz + f.lifted(g(), self.ks(MO), [0] * f.w)

    def affine(self, pt, ybound=MO):
        """exact limbs in [0, 2 p); ybound = MO + 1: y may be a negated table entry, limbs weakly normalised"""
        f = self.f
        return f.lifted(pt[0], self.ks(MO), [0] * f.w) + f.lifted(pt[1], self.ks(ybound), self.forms() if ybound > MO else [0] * f.w)


NEG_P_INV = (-pow(P, -1, 1 << 392)) % (1 << 392)


def redc(x):
    """The INTEGER a Montgomery reduction leaves for the column sum x: (x + m p) / 2^392 - somewhere in [0, 2 p).  Used only
    to find inputs whose intermediate products land in [p, 2 p), never for an expected result."""
    return (x + (x * NEG_P_INV % (1 << 392)) * P) >> 392


class _Steer:
    """The integers the first products of a formula of dev_curve.h leave, on G1 (w = 1) or G2 (w = 2)."""

    def __init__(self, w):
        self.w = w

    def mul(self, a, b):
        if self.w == 1:
            return [redc(a[0] * b[0])]
        return [redc(a[0] * b[0] + (16 * P - a[1]) * b[1]), redc(a[0] * b[1] + a[1] * b[0])]

    def sqr(self, a, bound):
        if self.w == 1:
            return [redc(a[0] * a[0])]
        return [redc((a[0] + a[1]) * (a[0] + (bound + 1) * P - a[1])), redc(2 * a[0] * a[1])]

    def subtrahends(self, op, row):
        """the products that enter a subtraction with the bound MO: {name: components}"""
        w = self.w
        v = [[val(s) for s in row[k * w:(k + 1) * w]] for k in range(len(row) // w)]
        sub = lambda a, b, bound: [x + (bound + 1) * P - y for x, y in zip(a, b)]
        if op in ("MDBL", "XDBL"):
            y = v[1]
            u = [2 * c for c in y]
            return {"w": self.mul(u, self.sqr(u, 2 * (MO + 1) if op == "MDBL" else 2 * BY))}
        if op in ("MADD", "MADD_NEG"):
            x, zz, px = v[0], v[2], v[4]
            pp_ = sub(self.mul(px, zz), x, BX)
            pp = self.sqr(pp_, MO + BX + 1)
            return {"ppp": self.mul(pp_, pp), "q": self.mul(x, pp)}
        x1, y1, zz1, x2, zz2, zzz2 = v[0], v[1], v[2], v[4], v[6], v[7]
        u1 = self.mul(x1, zz2)
        p_ = sub(self.mul(x2, zz1), u1, MO)
        pp = self.sqr(p_, 2 * MO + 1)
        # (q = u1 pp, a product of two products, reaches p about once in 10^4 rows: not looked for)
        return {"u1": u1, "s1": self.mul(y1, zzz2), "ppp": self.mul(p_, pp)}


def group_rows(name):
    """-> (rows, expected affine sums: None = infinity)"""
    g2 = name.startswith("G2")
    fld = _Field(g2)
    c, w = fld.curve, fld.w
    pts = _points(fld, 83 + g2)
    b = _Builder(fld, 89 + g2)
    rows, want = [], []
    op = name.split("_", 1)[1]
    aff = lambda P_, Q_: c.to_affine(c.add(c.to_jac(P_), c.to_jac(Q_)))
    dbl = lambda P_: c.to_affine(c.dbl(c.to_jac(P_)))
    if op == "MDBL":
        for p in pts:
            for _ in range(12):
                rows.append(b.affine(p, MO + 1))
                want.append(dbl(p))
    elif op == "XDBL":
        for p in pts:
            for _ in range(BX + 2):
                rows.append(b.xyzz(p))
                want.append(dbl(p))
            rows.append(b.xyzz(p, BX - 1, BY - 1))
            want.append(dbl(p))
        for _ in range(6):
            rows.append(b.infinity())
            want.append(None)
    elif op in ("MADD", "MADD_NEG"):
        neg = op == "MADD_NEG"
        eff = (lambda q: c.neg_affine(q)) if neg else (lambda q: q)      # the point the call adds
        for i, p in enumerate(pts):
            for j, q in enumerate(pts):
                if i == j:
                    continue
                for _ in range(3):
                    rows.append(b.xyzz(p) + b.affine(q))
                    want.append(aff(p, eff(q)))
            rows.append(b.xyzz(p, BX - 1, BY - 1) + b.affine(pts[(i + 1) % len(pts)]))
            want.append(aff(p, eff(pts[(i + 1) % len(pts)])))
            for _ in range(BX):
                # the accumulator is the addend under another representative: must double; its opposite: infinity
                rows.append(b.xyzz(eff(p)) + b.affine(p))
                want.append(dbl(eff(p)))
                rows.append(b.xyzz(c.neg_affine(eff(p))) + b.affine(p))
                want.append(None)
            for _ in range(3):
                rows.append(b.infinity() + b.affine(p))
                want.append(eff(p))
    else:   # XADD
        for i, p in enumerate(pts):
            for j, q in enumerate(pts):
                if i == j:
                    continue
                for _ in range(3):
                    rows.append(b.xyzz(p) + b.xyzz(q))
                    want.append(aff(p, q))
            rows.append(b.xyzz(p, BX - 1, BY - 1) + b.xyzz(pts[(i + 1) % len(pts)], BX - 1, BY - 1))
            want.append(aff(p, pts[(i + 1) % len(pts)]))
            for _ in range(BX):
                rows.append(b.xyzz(p) + b.xyzz(p))
                want.append(dbl(p))
                rows.append(b.xyzz(p) + b.xyzz(c.neg_affine(p)))
                want.append(None)
            for _ in range(2):
                rows.append(b.infinity() + b.xyzz(p))
                want.append(p)
                rows.append(b.xyzz(p) + b.infinity())
                want.append(p)
            rows.append(b.infinity() + b.infinity())
            want.append(None)
    # A product is "< 2 p", but on random inputs it is >= p about once in a hundred times, and the subtractions that take a
    # product with the bound MO are only exercised then: look for generic rows (top lifts) where each such product has a
    # component in [p, 2 p)
    steer = _Steer(w)
    make = {"MDBL": lambda p, q: (b.affine(p, MO + 1), dbl(p)), "XDBL": lambda p, q: (b.xyzz(p, BX - 1, BY - 1), dbl(p)),
            "MADD": lambda p, q: (b.xyzz(p, BX - 1, BY - 1) + b.affine(q), aff(p, q)),
            "MADD_NEG": lambda p, q: (b.xyzz(p, BX - 1, BY - 1) + b.affine(q), aff(p, c.neg_affine(q))),
            "XADD": lambda p, q: (b.xyzz(p, BX - 1, BY - 1) + b.xyzz(q, BX - 1, BY - 1), aff(p, q))}[op]
    found = set()
    walk = c.to_jac(pts[2])
    for tries in range(8000):
        p, q = pts[tries % 3], pts[3 + tries % 3]
        if op == "MDBL":        # an affine point has no z to vary: walk through the multiples of the generator
            walk = c.add(walk, c.to_jac(c.gen))
            p = c.to_affine(walk)
        row, e = make(p, q)
        hit = steer.subtrahends(op, row)
        for key, comps in hit.items():
            if max(comps) >= P and key not in found:
                found.add(key)
                rows.append(row)
                want.append(e)
        if len(found) == len(hit):
            break
    else:
        raise AssertionError("no row found whose products reach [p, 2 p): %s %s" % (name, found))
    # the preconditions: every coordinate inside its bound, ZZ / ZZZ / affine x exactly normalised
    nacc = {"MDBL": 0, "XDBL": 1, "MADD": 1, "MADD_NEG": 1, "XADD": 2}[op]
    for r in rows:
        for k in range(nacc):
            pt = r[4 * w * k:4 * w * (k + 1)]
            assert all(ratio(s) < BX for s in pt[:w]) and all(ratio(s) < BY for s in pt[w:2 * w])
            assert all(ratio(s) < MO and s == exact(val(s)) for s in pt[2 * w:])
            assert all(x <= WK for s in pt for x in s[:13])
        a = r[4 * w * nacc:]
        if a:
            assert len(a) == 2 * w and all(ratio(s) < MO and s == exact(val(s)) for s in a[:w])
            assert all(ratio(s) < (MO + 1 if op == "MDBL" else MO) and all(x <= WK for x in s[:13]) for s in a[w:])
            assert not (fld.is_zero(a[:w]) and fld.is_zero(a[w:]))        # an affine (0, 0) is outside the contract
    return rows, want


def check_group(lib, name):
    fld = _Field(name.startswith("G2"))
    F, w = fld.F, fld.w
    rows, want = group_rows(name)
    out, _ = run(lib, name, rows)
    n_inf = 0
    for i, (o, e) in enumerate(zip(out, want)):
        x, y, zz, zzz = (o[k * w:(k + 1) * w] for k in range(4))
        if e is None:
            assert fld.is_zero(zz), (name, i, "expected infinity")
            assert all(val(s) in (0, P) for s in zz), (name, i)
            n_inf += 1
            continue
        assert not fld.is_zero(zz), (name, i, "unexpected infinity")
        got = (F.mul(fld.plain(x), F.inv(fld.plain(zz))), F.mul(fld.plain(y), F.inv(fld.plain(zzz))))
        assert F.eq(got[0], e[0]) and F.eq(got[1], e[1]), (name, i)
        assert all(ratio(s) < BX for s in x) and all(ratio(s) < BY for s in y), (name, i)
        assert all(ratio(s) < MO and all(l < W for l in s[:13]) for s in zz + zzz), (name, i)
        assert all(l <= WK for s in x + y for l in s[:13]), (name, i)
    assert n_inf or name.endswith("MDBL")
    return len(rows)


# ------------------------------------------------------------------------------------------------ dispatch
def checker(name):
    if name.startswith(("G1_", "G2_")):
        return check_group
    if name.startswith(("FR_", "FQ32_")):
        return check_fp
    if name.startswith("FQ2X_"):
        return check_fq2x_linear if name.startswith(("FQ2X_ADD", "FQ2X_SUB_")) else check_fq2x_products
    if name in ("FQ28_MUL", "FQ28_SQR", "FQ28_MUL_RAW_10"):
        return check_fq28_mul
    if name.startswith("FQ28_MUL_SUB2_"):
        return check_fq28_mul_sub2
    if name in ("FQ28_CANON", "FQ28_WRED", "FQ28_IS_ZERO_FULL", "FQ28_IS_ZERO_LAZY"):
        return check_fq28_unary
    if name in ("FQ28_UNPACK", "FQ28_IMPORT", "FQ28_EXPORT"):
        return check_fq28_host
    return check_fq28_linear


def check_op(lib, name):
    """One hook call for the op; returns the number of rows it checked."""
    return checker(name)(lib, name)


def op_table_and_the_first_code_past_it(lib):
    """The C enum lists the names of OPS in their order (so the two tables have the same length; check_op reaches every code
    of it), and the first code past the table - past the row ops, which continue it - is refused without touching the
    output."""
    assert ops_of_the_c_source() == OP_NAMES
    past = len(OPS) + len(ops_of_the_c_source("ZK_HK_COOP_OPS"))     # the row ops (tests/coop_cases.py) continue the codes
    fn = lib.dll.zk_hook_field_op
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    a = np.zeros((1, 16, 16), dtype=np.uint32)
    out = np.full((1, 16, 16), 7, dtype=np.uint32)
    assert fn(len(OPS) - 1, a.ctypes.data, out.ctypes.data, 0) == 0
    assert fn(past - 1, a.ctypes.data, out.ctypes.data, 0) == 0
    assert fn(past, a.ctypes.data, out.ctypes.data, 1) == ZK_ERR_INVALID_ARGUMENT
    assert fn(0xffffffff, a.ctypes.data, out.ctypes.data, 1) == ZK_ERR_INVALID_ARGUMENT
    assert (out == 7).all()
