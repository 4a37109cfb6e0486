"""Cases for the wave-cooperative field and its group law (csrc/coop_field.h, csrc/coop_curve.h: one Fq element over the 16
lanes of a DPP row), shared by the emulation (CPU) and the GPU tests of tests/test_coop_field_ops.py.  The row ops of the
test hook zk_hook_field_op (csrc/field_hooks.cpp, the COOP_* codes that continue enum FieldOp) get rows of operands whose
limbs the builder chooses one by one - the operands, limb forms, margins and output contracts of tests/field_cases.py - and
every output row is compared with Python integers / oracle/bls12_381.py and with the contract the header states for it.

A GPU wave holds FOUR rows.  Every launch is at least one full wave and a partial one (a row count that is no multiple of
4), and the rows of a case list are sent in a strided order, so that the four rows of a wave come from four distant parts of
the list: different magnitudes, different limb forms, different branches of the group law.  A builder asserts the
preconditions of its op (the inequalities of the ZK_FQ28_CHECK lines, the limb bound of raw operands) on every row before it
is sent; the emulation build, where those lines and the abort on non-zero lanes 14 / 15 are live, proves them."""
from fractions import Fraction

import field_cases as fc
from field_cases import (BX, BY, EPS, MARGIN, MASK, MO, P, P13, R392, RINV, W, WK, exact, largest_k, mont, operands, pattern, pick,
                         ratio, raw_operand, spread, sprinkled, val, weak, words32)
from oracle import synth

WAVE = 4                                                            # rows of a GPU wave
BS = (2, 4, 5, 7, 8, 9, 10, 14, 15, 16, 18, 32, 35, 63)             # sub_b / neg_b bounds of the row kernels, and the last constant
SQR_AS = (2, 4, 5, 6, 7, 8, 9, 10)                                  # coop_slot_sqr<A>, sqr = sqr_b<4>
# coop_products<K, NT, MASK> as the group law instantiates it
SHAPES = {"COOP_PRODUCTS_3_2": (3, 2, 0b010111), "COOP_PRODUCTS_2_2": (2, 2, 0b0111), "COOP_PRODUCTS_6_1": (6, 1, 0b111111),
          "COOP_PRODUCTS_6_2": (6, 2, 0b010111111111), "COOP_PRODUCTS_8_2": (8, 2, (1 << 16) - 1), "COOP_PRODUCTS_12_2": (12, 2, (1 << 24) - 1)}
# public exponents of the row kernels (csrc/consts.h): q - 2, (q + 1) / 4, (q - 3) / 4, (q - 1) / 2
PUBLIC_EXPONENTS = (P - 2, (P + 1) // 4, (P - 3) // 4, (P - 1) // 2)


def _op_table():
    t = [("COOP_FQ_ADD", 2, 1), ("COOP_FQ_DBL", 1, 1)]
    for b in BS:
        t += [("COOP_FQ_SUB_B_%d" % b, 2, 1), ("COOP_FQ_NEG_B_%d" % b, 1, 1), ("COOP_FQ_SUB_RAW_%d" % b, 2, 1), ("COOP_FQ_NEG_RAW_%d" % b, 1, 1),
              ("COOP_FQ2_SUB_B_%d" % b, 4, 2)]
    t += [("COOP_FQ_SUB_SUB2_2_2", 3, 1), ("COOP_FQ_MUL", 2, 1), ("COOP_FQ_SQR", 1, 1), ("COOP_FQ_MUL2", 4, 2), ("COOP_FQ_MUL_SUB2_2", 4, 1),
          ("COOP_FQ_MUL_SUB2_5", 4, 1), ("COOP_FQ_MUL_RAW_10", 3, 1), ("COOP_FQ_WNORM", 1, 1), ("COOP_FQ_EXACT", 1, 1),
          ("COOP_FQ_IS_ZERO_NORM", 1, 1), ("COOP_FQ_IS_ZERO_FULL", 1, 1)]
    t += [(n, 2 * k * nt, k) for n, (k, nt, _) in SHAPES.items()]
    t += [("COOP_FQ2_ADD", 4, 2), ("COOP_FQ2_SUB_SUB2_2_2", 6, 2), ("COOP_FQ2_MUL", 4, 2)]
    t += [("COOP_FQ2_SQR_B_%d" % a, 2, 2) for a in SQR_AS]
    t += [("COOP_FQ2_IS_ZERO_NORM", 2, 1), ("COOP_FQ2_IS_ZERO_FULL", 2, 1), ("COOP_GATHER_SCATTER", 1, 1), ("COOP_UNPACK", 1, 1),
          ("COOP_IMPORT", 1, 1), ("COOP_IMPORT_PLAIN", 1, 1), ("COOP_EXPORT", 1, 1), ("COOP_POW", 2, 1), ("COOP_INV_FERMAT", 1, 1),
          ("COOP_INV", 1, 1), ("COOP_LEX_LARGEST", 1, 1)]
    t += [("COOP_G1_XDBL", 4, 4), ("COOP_G1_XADD", 8, 4), ("COOP_G1_XDBL_XADD", 8, 4), ("COOP_G1_MADD", 6, 4)]
    t += [("COOP_G2_XDBL", 8, 8), ("COOP_G2_XADD", 16, 8), ("COOP_G2_XDBL_XADD", 16, 8)]
    return t


OPS = _op_table()               # the order of enum CoopFieldOp in csrc/field_hooks.cpp; its codes continue those of FieldOp
OP_NAMES = [n for n, _, _ in OPS]
OP_CODE = {n: len(fc.OPS) + i for i, n in enumerate(OP_NAMES)}


# ------------------------------------------------------------------------------------------------ the hook
def strided(items):
    """The list in an order whose neighbours lie about 0.38 of its length apart (a stride coprime to the length)."""
    n = len(items)
    s = max(1, int(n * 0.381966))
    while n > 1 and _gcd(s, n) != 1:
        s += 1
    return [items[(i * s) % n] for i in range(n)]


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def run(lib, name, rows, in_order=False):
    """-> (output slots per row, the rows as sent).  The rows go out in the strided order unless the caller has ordered
    them itself (in_order: the group law, whose expected points are a second list)."""
    _, ni, no = OPS[OP_CODE[name] - len(fc.OPS)]
    return fc.launch(lib, name, OP_CODE[name], ni, no, rows if in_order else strided(list(rows)), WAVE)


def via(name):
    """The run function a checker of field_cases.py takes, sending its rows through the row op `name`."""
    return lambda lib, _twin, rows: run(lib, name, rows)


def assert_product(l, want_residue, what):
    """a product on rows: weakly normalised, < 2 p, the right residue"""
    fc.assert_weak(l, what)
    v = val(l)
    assert v < 2 * P, (what, hex(v))
    assert v % P == want_residue % P, (what, hex(v))


def truth(o):
    assert o[0][1:] == [0] * 13 and o[0][0] in (0, 1), o
    return o[0][0]


# ------------------------------------------------------------------------------------------------ carry passes, zero tests
def from_carries(u, c):
    """Limbs t whose carry-save pass (coop_wnorm) leaves exactly the limbs u: c[j] is the carry limb j hands up."""
    t = []
    for j in range(14):
        low = u[j] - (c[j - 1] if j else 0)
        assert 0 <= low <= MASK and (c[j] == 0 or j < 13), (j, u, c)
        t.append(c[j] * W + low)
    assert val(t) == val(u)
    return t


def carry_runs(rng, raw):
    """(limbs, what) whose carry-save pass leaves a generated carry (a limb at 2^28) directly below a run of 2^28 - 1 limbs.
    Lane 0 receives no carry, so the lowest generating limb is limb 1; the carry a run passes on must land in a limb (the
    value is below 2^392), so a run that a carry enters has length 1 .. 11 and the longest one ends in limb 12, its carry
    in limb 13.  Runs of length 12 and 13 and the runs that include limb 13 exist only with NO carry entering them.
    raw: carries up to 4 per limb, as in the limbs sub_raw leaves; otherwise weakly normalised limbs."""
    out = []

    def build(gens, runs, what):
        u = [9 + rng.below(MASK - 10) for _ in range(13)] + [rng.below(P13)]      # the limbs after the pass: none 2^28 - 1
        c = [(rng.below(5) if raw else 0) for _ in range(13)] + [0]               # what each limb hands up in the pass
        for g in gens:
            u[g] = W
            c[g - 1] = 1 + rng.below(4) if raw else 1
            if not raw:                                  # a weak limb that hands a carry up is 2^28 + 0 .. 8
                u[g - 1] = rng.below(9)
        for lo, hi in runs:
            for j in range(lo, hi + 1):
                assert not (c[j] and not raw)
                u[j] = MASK
        t = from_carries(u, c)
        assert all(x <= WK for x in t[:13]) or raw
        assert all(x < fc.RAW_LIMB_BOUND for x in t) and val(t) < (1 << 392)
        out.append((t, what))

    for length in range(1, 12):
        for g in range(1, 13 - length):
            build([g], [(g + 1, g + length)], ("carry into a run", g, length))
    for g1, l1, g2, l2 in ((1, 1, 4, 1), (1, 3, 7, 5), (2, 4, 8, 4), (1, 5, 8, 4), (3, 1, 6, 6), (1, 1, 4, 8)):
        build([g1, g2], [(g1 + 1, g1 + l1), (g2 + 1, g2 + l2)], ("two runs", g1, l1, g2, l2))
    for lo, hi in ((0, 0), (0, 12), (0, 13), (1, 13), (5, 13), (13, 13), (3, 9), (12, 13)):
        build([], [(lo, hi)], ("a run no carry enters", lo, hi))
    build([3], [(6, 9)], ("a carry and a run apart", 3, 6, 9))
    build([2, 3] if raw else [2], [(5, 5)], ("generators side by side", 2))
    return out


def raw_results(rng, n=60):
    """Limbs as sub_raw<B> leaves them (a + the spread form of (B + 1) p - b, no carry pass), computed here."""
    out = []
    for i in range(n):
        b = BS[i % len(BS)]
        lb, la = operands(b), operands(64 - b - 1) if b < 63 else [exact(0)]
        x, y = (pick(la, i, 5, 2), pick(lb, i, 3, 1)) if i % 3 else (la[-1], exact(0) if b < 63 else lb[-1])
        sp = spread(b + 1)
        t = [x[j] + sp[j] - y[j] for j in range(14)]
        assert all(0 <= l < fc.RAW_LIMB_BOUND for l in t) and val(t) < 64 * P
        out.append(t)
    return out


def rows_exact():
    rng = synth.SplitMix64(211)
    rows = [[t] for t, _ in carry_runs(rng, False)] + [[t] for t, _ in carry_runs(rng, True)]
    rows += [[a] for a in operands(64)[::5]] + [[t] for t in raw_results(rng)]
    rows += [[exact(P)], [weak(P)], [exact(0)], [pattern(0)], [[MASK] * 14]]
    return rows


def rows_zero_norm():
    """Weakly normalised values below 2 p: 0 and p in every limb form, the near misses, and what lies around them."""
    rng = synth.SplitMix64(223)
    zeros = [exact(0), exact(P), weak(P)]            # (no limb of p is 0 .. 8: p and 0 have ONE weakly normalised form each)
    near = [val(sprinkled(P, rng)) for _ in range(6)] + [val(sprinkled(0, rng)) for _ in range(3)]     # limbs at 2^28 + 0 .. 8
    near += [1, P - 1, P + 1, 2 * P - 1 - EPS] + [1 << (28 * k) for k in range(1, 14)] + [P + (1 << (28 * k)) for k in range(1, 13)]
    near += [P - (1 << (28 * k)) for k in range(1, 14)] + [P ^ (1 << 380)]
    rows = []
    for i in range(8):
        rows += [[z] for z in zeros]                                 # (truth is not the rare case of a wave)
        for v in near[i::8]:
            rows += [[exact(v)], [weak(v)]]
    rows += [[exact(v)] for v in near] + [[a] for a in operands(2)]
    # p with ONE limb changed, in every lane: the ballot must see each lane
    for k in range(14):
        for d in (-1, 1):
            l = exact(P)
            l[k] += d
            rows.append([l])
        rows.append([[x if j == k else 0 for j, x in enumerate(exact(P))]])
        rows.append([[1 if j == k else 0 for j in range(14)]])
    for r in rows:
        assert ratio(r[0]) < 2 and all(x <= WK for x in r[0][:13])
    return rows


def check_carry(lib, name):
    if name == "COOP_FQ_WNORM":
        # any 32-bit limbs whose value is below 2^392: the value is kept, a limb takes what its lower neighbour hands up
        rng = synth.SplitMix64(227)
        rows = [[a] for a in operands(64)[::7]] + [[t] for t in raw_results(rng)] + [[t] for t, _ in carry_runs(rng, True)]
        rows += [[[0xffffffff] * 13 + [MASK - 16]], [[0xffffffff] * 13 + [0]], [[9 * W - 1] * 13 + [3]], [[8 * WK] * 13 + [8 * P13]]]
        for k in range(1, 9):                                        # sums of k weak values, no carry pass in between
            rows.append([[k * x for x in pattern(P13)]])
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            t = r[0]
            assert val(t) < (1 << 392)
            assert val(o[0]) == val(t), (name, r)
            for j in range(14):
                assert o[0][j] == (t[j] & MASK) + ((t[j - 1] >> 28) if j else 0), (name, j, r)
            if all(x < 9 * W for x in t):                            # additions / subtractions / a product's last round
                fc.assert_weak(o[0], (name, r))
    elif name == "COOP_FQ_EXACT":
        out, rows = run(lib, name, rows_exact())
        for r, o in zip(rows, out):
            assert o[0] == exact(val(r[0])), (name, r, o)
    elif name == "COOP_FQ_IS_ZERO_NORM":
        out, rows = run(lib, name, rows_zero_norm())
        for r, o in zip(rows, out):
            assert truth(o) == int(val(r[0]) in (0, P)), (name, r)
        assert 16 <= sum(truth(o) for o in out) <= len(out) - 16
    elif name == "COOP_FQ2_IS_ZERO_NORM":
        z = rows_zero_norm()
        rows = [[z[i][0], z[(i * 3 + 1) % len(z)][0]] for i in range(len(z))]
        zs = [r[0] for r in z if val(r[0]) in (0, P)]
        rows += [[a, b] for a in zs[:5] for b in zs[:5]]
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            assert truth(o) == int(val(r[0]) in (0, P) and val(r[1]) in (0, P)), (name, r)
        assert 16 <= sum(truth(o) for o in out) <= len(out) - 16
    else:   # COOP_GATHER_SCATTER: the identity on limbs, whatever they hold
        rng = synth.SplitMix64(229)
        rows = [[a] for a in operands(64)[::9]] + [[[0xffffffff] * 14], [[0] * 14], [[(j + 1) * 0x11111111 & 0xffffffff for j in range(14)]]]
        rows += [[[rng.below(1 << 32) for _ in range(14)]] for _ in range(40)]
        rows += [[[0xffffffff if j == k else 0 for j in range(14)]] for k in range(14)]
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            assert o[0] == list(r[0]), (name, r)
    return len(rows)


# ------------------------------------------------------------------------------------------------ products
def check_mul2(lib, name):
    base = fc.rows_mul()
    n = len(base)
    rows = [base[i] + base[(i * 5 + 3) % n] for i in range(n)]
    out, rows = run(lib, name, rows)
    for r, o in zip(rows, out):
        assert_product(o[0], mont(val(r[0]) * val(r[1])), (name, 0, r))
        assert_product(o[1], mont(val(r[2]) * val(r[3])), (name, 1, r))
    return len(rows)


def rows_products(k_acc, nt, mask):
    """Rows of 2 K NT slots: the x of (accumulator k, term t) in slot k NT + t, its y in slot K NT + k NT + t.  The x enter
    limb-wise (weak, or raw as sub_raw / neg_raw leave them), the y by broadcast (weak).  Every accumulator and every term
    gets operands of its own - the terms outside the mask too, which must not count - and the live terms of an accumulator
    share its budget: |x| |y| < 2500 p^2 for one term (mul), the sum < 2000 p^2 for two (mul_sub2, the Fq2 product)."""
    rng = synth.SplitMix64(233 + 16 * k_acc + nt)
    live = [[t for t in range(nt) if (mask >> (k * nt + t)) & 1] for k in range(k_acc)]
    assert all(live)
    xs = operands(13) + [raw_operand(b, top) for b in (2, 5, 10, 15) for top in (0, P13, 20 * P13)]
    rows = []

    def row(choose):
        x = [[None] * nt for _ in range(k_acc)]
        y = [[None] * nt for _ in range(k_acc)]
        for k in range(k_acc):
            budget = Fraction(2500 if len(live[k]) == 1 else 2000, len(live[k]))
            for t in range(nt):
                x[k][t], y[k][t] = choose(k, t, budget) if t in live[k] else (pick(operands(4), rng.below(1000)), pick(operands(4), rng.below(1000)))
        rows.append([x[k][t] for k in range(k_acc) for t in range(nt)] + [y[k][t] for k in range(k_acc) for t in range(nt)])

    def generic(form):
        def choose(k, t, budget):
            xv = pick(xs, rng.below(100000), 1, 0)
            ky = largest_k(budget, ratio(xv))
            if ky < 0:
                xv, ky = pick(operands(13), rng.below(1000)), largest_k(budget, 13)
            f = (form + k + t) % 4
            yv = [exact(ky * P + P - 1), pattern(max(0, ky * P13 - 2)), sprinkled(rng.below(ky + 1) * P + rng.field(P), rng), exact(rng.field(P))][f]
            if ratio(yv) >= ky + 1:
                yv = exact(ky * P + rng.field(P))
            return xv, yv
        return choose

    for i in range(40):
        row(generic(i))
    # x limbs at the raw bound in every live term, y limbs at 2^28 + 8 in every lane, at the largest tops the budget admits
    for b, top in ((10, 0), (10, P13), (15, 0), (2, 3 * P13), (5, 30 * P13)):
        def at_the_bound(k, t, budget):
            xv = raw_operand(b, top)
            ymax = min(int((budget - 2 * MARGIN) * P * P / val(xv)), 64 * P - EPS)       # |x| |y| just under the budget
            assert ymax >= fc.LOW_WK
            return xv, pattern((ymax - fc.LOW_WK) >> 364)
        row(at_the_bound)
    # an accumulator that lands on 0 or on p: multiples of p, and two terms that cancel mod p (x1 = m p - x0, y1 = y0)
    for i in range(12):
        def cancels(k, t, budget):
            yv = pick(operands(12), i + k, 7, 1)
            x0 = pick(operands(6), i + 3 * k, 5, 2)
            m = (val(x0) + P - 1) // P + (i + k) % 3
            if len(live[k]) == 1:
                return exact(((i + k) % 12) * P), yv
            return (x0, yv) if t == live[k][0] else (exact(m * P - val(x0)), yv)
        row(cancels)
    for r in rows:
        n = k_acc * nt
        for k in range(k_acc):
            s = sum(ratio(r[k * nt + t]) * ratio(r[n + k * nt + t]) for t in live[k])
            assert s <= (2500 if len(live[k]) == 1 else 2000) - MARGIN, (k, float(s))
        assert all(x < fc.RAW_LIMB_BOUND for s in r[:n] for x in s[:13]) and all(x <= WK for s in r[n:] for x in s[:13])
        assert all(ratio(s) < 64 for s in r)
    return rows, live


def check_products(lib, name):
    k_acc, nt, mask = SHAPES[name]
    rows, live = rows_products(k_acc, nt, mask)
    out, rows = run(lib, name, rows)
    n = k_acc * nt
    landed = 0
    for r, o in zip(rows, out):
        for k in range(k_acc):
            s = sum(val(r[k * nt + t]) * val(r[n + k * nt + t]) for t in live[k])
            assert_product(o[k], mont(s), (name, k, r))
            landed += val(o[k]) in (0, P)
    assert landed >= k_acc
    return len(rows)


# ------------------------------------------------------------------------------------------------ chains
def stored(v, k, form):
    """the plain value v in Montgomery form at the magnitude k p + r, limbs exact (form 0) or weak"""
    s = v * R392 % P + k * P
    return weak(s) if form else exact(s)


def exponents():
    e = [0, 1, 2, 15, 16, (1 << 384) - 1, 1 << 383, 1 << 380, 3 << 382]
    rng = synth.SplitMix64(239)
    for w in range(1, 12):
        for s in (2, 1, 0):                     # a window of width four from bit 32 w + s: 1, 2, 3 bits from the lower word
            b = 32 * w + s
            win = (1 << b) | (1 << (b - 3))
            e.append(win)
            above = ((rng.below(1 << 20) | 1) << (b + 5)) if b + 25 <= 383 else 0      # (bits b + 1 .. b + 4 stay clear)
            e.append(above | win | (1 << (b - 1)) | rng.below(1 << (b - 4)))
        # ... cut short by trailing zeros: it ends on the boundary, one bit above it, or one and two bits below it
        e += [(3 << (32 * w)), (1 << (32 * w + 1)), (5 << (32 * w - 2)) | 1, (3 << (32 * w - 1)) | (1 << (32 * w - 9)), (1 << (32 * w)) | 7]
    for s in (2, 1, 0):                         # the bottom of word 0: a window of 3, 2, 1 bits
        e += [(1 << 200) | ((1 << (s + 1)) - 1), (1 << 40) | (1 << s), (1 << 7) | (1 << s)]
    e += [(1 << 383) | 1, (15 << 380) | (1 << 190) | 9, (9 << 300) | (1 << 33), (1 << 64) | (1 << 31)]       # long runs of zeros
    e += list(PUBLIC_EXPONENTS)
    e += [rng.field(1 << 384) for _ in range(6)]
    assert all(0 <= x < (1 << 384) for x in e)
    return e


def check_chain(lib, name):
    rng = synth.SplitMix64(241)
    if name == "COOP_POW":
        bases = [0, 1, P - 1, 2] + [rng.field(P) for _ in range(4)]
        rows, i = [], 0
        for e in exponents():
            for _ in range(2):
                i += 1
                k = (49, 0, 1, 30, 48, 7)[i % 6]                     # a^2 is a product: the base stays below 50 p
                a = stored(bases[i % len(bases)], k, i % 2)
                if ratio(a) ** 2 > 2500 - MARGIN:
                    a = exact(50 * P - EPS)
                rows.append([a, words32(e)])
        rows.append([exact(50 * P - EPS), words32(PUBLIC_EXPONENTS[0])])
        for r in rows:
            assert ratio(r[0]) ** 2 <= 2500 - MARGIN and all(x <= WK for x in r[0][:13])
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            e = sum(w << (32 * j) for j, w in enumerate(r[1]))
            a = val(r[0]) * RINV % P
            got = val(o[0])
            fc.assert_weak(o[0], (name, r))
            assert got % P == pow(a, e, P) * R392 % P, (name, hex(e), r[0])
            assert got < max(2 * P, val(r[0]) + 1), (name, hex(e))     # (e == 1: the base itself comes back)
    elif name in ("COOP_INV", "COOP_INV_FERMAT"):
        import parity_cases
        vs = parity_cases.fq_inverse_edge_values() + [rng.field(P) for _ in range(20)]
        rows = []
        for i, v in enumerate(vs):
            for k in sorted({0, 1, (i * 7) % 50, 49}):
                rows.append([stored(v, k, (i + k) % 2)])
        rows += [[exact(k * P)] for k in range(50)] + [[weak(k * P)] for k in (1, 2, 17, 49)]      # k p -> 0
        rows = [r for r in rows if ratio(r[0]) ** 2 <= 2500 - MARGIN]
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            a = val(r[0]) * RINV % P
            assert_product(o[0], pow(a, P - 2, P) * R392, (name, r))
    else:   # COOP_LEX_LARGEST
        vs = [(P - 1) // 2, (P + 1) // 2, 0, 1, P - 1, 2, (P - 3) // 2, (P + 3) // 2] + [rng.field(P) for _ in range(6)]
        vs += [(P - 1) // 2 + d for d in (1 << 28, -(1 << 28), 1 << 364, -(1 << 364), 1 << 196)]
        rows = []
        for i, v in enumerate(vs):
            for k in range(64):
                if i < 5 or k in (0, 1, 63, (i * 11) % 64):
                    s = v * R392 % P + k * P
                    rows.append([exact(s)])
                    if weak(s) != exact(s) and (i < 5 or k % 2):
                        rows.append([weak(s)])
        rows += [[exact(k * P)] for k in range(64)] + [[weak(k * P)] for k in range(1, 64, 3)]    # the residue p itself
        for r in rows:
            assert ratio(r[0]) <= 64 - MARGIN and all(x <= WK for x in r[0][:13])
        out, rows = run(lib, name, rows)
        for r, o in zip(rows, out):
            assert truth(o) == int(val(r[0]) * RINV % P > (P - 1) // 2), (name, r)
        assert 64 <= sum(truth(o) for o in out) <= len(out) - 64
    return len(rows)


def check_import(lib, name):
    """12 host words -> a row in Montgomery form, words of every value below 2^384 (at or above q too: unpack does no
    arithmetic, and the product that follows takes any of them).  COOP_IMPORT: x 2^384 -> x 2^392, the product with KIN =
    2^400; COOP_IMPORT_PLAIN: the plain x -> x 2^392, the product with R2 = 2^784."""
    factor = 256 if name == "COOP_IMPORT" else R392
    out, rows = run(lib, name, [[words32(v)] for v in fc.host_values() + [(1 << 384) - 1, (1 << 384) - (1 << 32), 1 << 383, P, P + 1, 9 * P]])
    for r, o in zip(rows, out):
        m = sum(w << (32 * i) for i, w in enumerate(r[0]))
        assert_product(o[0], m * factor, (name, r))
    return len(rows)


# ------------------------------------------------------------------------------------------------ the group law
def _weak_zz(rows, w, npts):
    """ZZ and ZZZ of every other row in weak form: on rows they are products, weakly normalised (one-lane: exact)."""
    out = []
    for i, r in enumerate(rows):
        r = list(r)
        if i % 2:
            for k in range(npts):
                for s in range(4 * w * k + 2 * w, 4 * w * (k + 1)):
                    r[s] = weak(val(r[s]))
        out.append(r)
    return out


def composite_rows(g2):
    """xadd(xdbl(a), b): generic, b = 2 a (the addition finds equal points and doubles), b = -2 a, either at infinity"""
    fld = fc._Field(g2)
    c = fld.curve
    pts = fc._points(fld, 97 + g2)
    b = fc._Builder(fld, 101 + g2)
    dbl = lambda p: c.to_affine(c.dbl(c.to_jac(p)))
    aff = lambda p, q: c.to_affine(c.add(c.to_jac(p), c.to_jac(q)))
    rows, want = [], []
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            if dbl(p) == q or c.neg_affine(dbl(p)) == q:
                continue
            for _ in range(2):
                rows.append(b.xyzz(p) + b.xyzz(q))
                want.append(aff(dbl(p), q))
        rows.append(b.xyzz(p, BX - 1, BY - 1) + b.xyzz(pts[(i + 2) % len(pts)], BX - 1, BY - 1))
        want.append(aff(dbl(p), pts[(i + 2) % len(pts)]))
        for _ in range(4):
            rows.append(b.xyzz(p) + b.xyzz(dbl(p)))
            want.append(dbl(dbl(p)))
            rows.append(b.xyzz(p) + b.xyzz(c.neg_affine(dbl(p))))
            want.append(None)
        for _ in range(2):
            rows.append(b.infinity() + b.xyzz(p))
            want.append(p)
            rows.append(b.xyzz(p) + b.infinity())
            want.append(dbl(p))
        rows.append(b.infinity() + b.infinity())
        want.append(None)
    return rows, want


def check_group(lib, name):
    g2 = name.startswith("COOP_G2")
    fld = fc._Field(g2)
    F, w = fld.F, fld.w
    op = name.split("_", 2)[2]
    if op == "XDBL_XADD":
        rows, want = composite_rows(g2)
    else:
        rows, want = fc.group_rows(("G2_" if g2 else "G1_") + op)
    npts = {"XDBL": 1, "MADD": 1, "XADD": 2, "XDBL_XADD": 2}[op]
    rows = _weak_zz(rows, w, npts)
    for r in rows:      # the preconditions: X < BX p, Y < BY p, ZZ and ZZZ < MO p, weak limbs; an affine addend below MO p
        for k in range(npts):
            pt = r[4 * w * k:4 * w * (k + 1)]
            assert all(ratio(s) < BX for s in pt[:w]) and all(ratio(s) < BY for s in pt[w:2 * w]) and all(ratio(s) < MO for s in pt[2 * w:])
        assert all(ratio(s) < MO for s in r[4 * w * npts:]) and all(x <= WK for s in r for x in s[:13])
    order = strided(list(range(len(rows))))
    out, sent = run(lib, name, [rows[i] for i in order], in_order=True)
    want = [want[order[i % len(order)]] for i in range(len(sent))]
    assert all(sent[i] == rows[order[i % len(order)]] for i in range(len(sent)))
    n_inf = 0
    for i, (o, e) in enumerate(zip(out, want)):
        x, y, zz, zzz = (o[k * w:(k + 1) * w] for k in range(4))
        if e is None:
            assert all(val(s) in (0, P) for s in zz), (name, i, "expected infinity")
            n_inf += 1
            continue
        assert not fld.is_zero(zz), (name, i, "unexpected infinity")
        got = (F.mul(fld.plain(x), F.inv(fld.plain(zz))), F.mul(fld.plain(y), F.inv(fld.plain(zzz))))
        assert F.eq(got[0], e[0]) and F.eq(got[1], e[1]), (name, i)
        assert all(ratio(s) < BX for s in x) and all(ratio(s) < BY for s in y) and all(ratio(s) < MO for s in zz + zzz), (name, i)
        assert all(l <= WK for s in o for l in s[:13]), (name, i)
    assert n_inf
    # the four rows of a wave differ: no wave of one expectation only
    kinds = [None if e is None else 1 for e in want]
    assert any(len(set(kinds[i:i + WAVE])) > 1 for i in range(0, len(kinds) - WAVE, WAVE))
    return len(sent)


# ------------------------------------------------------------------------------------------------ dispatch
def _twin(name):
    """(the checker of field_cases.py, the one-lane name it reads its bound from) for the ops that have a one-lane twin"""
    if name.startswith("COOP_FQ2_"):
        t = "FQ2X_" + name[len("COOP_FQ2_"):]
        return (fc.check_fq2x_linear if t.startswith(("FQ2X_ADD", "FQ2X_SUB_")) else fc.check_fq2x_products), t
    if name in ("COOP_UNPACK", "COOP_EXPORT"):
        return fc.check_fq28_host, "FQ28_" + name[len("COOP_"):]
    t = "FQ28_" + name[len("COOP_FQ_"):]
    if t in ("FQ28_MUL", "FQ28_SQR", "FQ28_MUL_RAW_10"):
        return fc.check_fq28_mul, t
    if t.startswith("FQ28_MUL_SUB2_"):
        return fc.check_fq28_mul_sub2, t
    if t == "FQ28_IS_ZERO_FULL":
        return fc.check_fq28_unary, t
    assert t.startswith(("FQ28_ADD", "FQ28_DBL", "FQ28_SUB_", "FQ28_NEG_")), name
    return fc.check_fq28_linear, t


def checker(name):
    if name.startswith(("COOP_G1_", "COOP_G2_")):
        return check_group
    if name in ("COOP_FQ_WNORM", "COOP_FQ_EXACT", "COOP_FQ_IS_ZERO_NORM", "COOP_FQ2_IS_ZERO_NORM", "COOP_GATHER_SCATTER"):
        return check_carry
    if name == "COOP_FQ_MUL2":
        return check_mul2
    if name in SHAPES:
        return check_products
    if name in ("COOP_POW", "COOP_INV_FERMAT", "COOP_INV", "COOP_LEX_LARGEST"):
        return check_chain
    if name in ("COOP_IMPORT", "COOP_IMPORT_PLAIN"):
        return check_import
    check, twin = _twin(name)
    if check in (fc.check_fq28_linear, fc.check_fq28_unary, fc.check_fq2x_linear):
        return lambda lib, n: check(lib, twin, run=via(n))
    # the one-lane twin's cases and expected residues; a product on rows is weakly, not exactly, normalised
    return lambda lib, n: check(lib, twin, run=via(n), assert_product=assert_product)


def check_op(lib, name):
    """One hook call for the op; returns the number of rows it sent."""
    return checker(name)(lib, name)


def op_table_and_the_first_code_past_it(lib):
    """The row ops of the C source are OPS in their order, after the one-lane table; the last code is taken and the first
    one past it refused without touching the output."""
    import ctypes as C
    import numpy as np
    assert fc.ops_of_the_c_source("ZK_HK_COOP_OPS") == OP_NAMES
    assert fc.ops_of_the_c_source() == fc.OP_NAMES and not set(OP_NAMES) & set(fc.OP_NAMES)
    fn = lib.dll.zk_hook_field_op
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    a = np.zeros((1, 48, 16), dtype=np.uint32)
    out = np.full((1, 48, 16), 7, dtype=np.uint32)
    past = len(fc.OPS) + len(OPS)
    assert fn(past - 1, a.ctypes.data, out.ctypes.data, 0) == 0
    assert fn(past, a.ctypes.data, out.ctypes.data, 1) == fc.ZK_ERR_INVALID_ARGUMENT
    assert (out == 7).all()
