"""Cases for the steps of the line preparation on rows (csrc/coop_verify.cpp: cv_double_step, cv_add_step on one row,
cvq_double_step, cvq_add_step on four rows per point), shared by the emulation (CPU) and the GPU tests of
tests/test_cv_line_steps.py, through the test hook zk_hook_cv_step: the running point (X, Y, Z) and, for an addition, x_Q, y_Q
and y_Q^2 arrive as slots of limbs the builder chooses, and X3, Y3, Z3 and the line (a, b, c) come back as the step leaves them.

The reference is the closed form of pairing.h's g2_double_step / g2_add_step over Fq2 in Python integers, in the reference's
scaling:
    doubling   E = 3 X^2:  X3 = E^2 - 8 X Y^2,  Z3 = 2 Y Z,  Y3 = E (4 X Y^2 - X3) - 8 Y^4,
               a = 2 Z3 Z^2,  b = -2 E Z^2,  c = 6 X^3 - 4 Y^2
    addition   H = x_Q Z^2 - X, r2 = 2 (y_Q Z^3 - Y):  X3 = r2^2 - 4 H^3 - 8 X H^2,  Z3 = 2 Z H,  Y3 = r2 (4 X H^2 - X3) - 8 Y H^3,
               a = 2 Z3,  b = -2 r2,  c = 2 r2 x_Q - 2 y_Q Z3
and for the points on the twist the new point is compared with the group law of oracle/bls12_381.py as well.  The formulas are
polynomial identities, so they also hold for coordinates that are no point of the curve: those cases put EVERY component at the
edge of its bound (one-row forms: X, Y, Z below 2 p; four-row forms: Z below 4 p; x_Q, y_Q below 2 p; y_Q^2, which the step
trusts, is the square in either representative), which the
coordinates of a point - residues the point dictates - reach in their representative and in Z only.

The line's contract with its consumer: k_c12_miller (coop_pairing.cpp) reads the stage unreduced - the constant term c enters
c12_line as it is, which budgets it below 64 p; a and b enter coop_products<4, 1> limb-wise against p_x, p_y below 2 p, which
under the 2000 p^2 budget of coop_field.h allows them below 1000 p, limbs weakly normalised."""
import ctypes as C

import numpy as np

import c12_cases as c12
import coop_cases as cc
import field_cases as fc
from field_cases import EPS, P, RINV, val
from oracle import bls12_381 as bls
from oracle import synth

F2 = bls.Fq2Ops
G2 = bls.G2
# the order of ZK_HK_CV_OPS in csrc/coop_verify.cpp: (name, slots in)
OPS = [("CV_DOUBLE_STEP", 6), ("CV_ADD_STEP", 12), ("CVQ_DOUBLE_STEP", 6), ("CVQ_ADD_STEP", 12)]
OP_NAMES = [n for n, _ in OPS]
OP_CODE = {n: i for i, n in enumerate(OP_NAMES)}
WAVE = 4


# ------------------------------------------------------------------------------------------------ the reference
def k2(k, a):
    return (k * a[0] % P, k * a[1] % P)


def ref_double(X, Y, Z):
    E = k2(3, F2.sqr(X))
    YY, ZZ = F2.sqr(Y), F2.sqr(Z)
    XYY = F2.mul(X, YY)
    X3 = F2.sub(F2.sqr(E), k2(8, XYY))
    Z3 = k2(2, F2.mul(Y, Z))
    Y3 = F2.sub(F2.mul(E, F2.sub(k2(4, XYY), X3)), k2(8, F2.sqr(YY)))
    a = k2(2, F2.mul(Z3, ZZ))
    b = F2.neg(k2(2, F2.mul(E, ZZ)))
    c = F2.sub(k2(6, F2.mul(F2.sqr(X), X)), k2(4, YY))
    return X3, Y3, Z3, a, b, c


def ref_add(X, Y, Z, qx, qy):
    ZZ = F2.sqr(Z)
    H = F2.sub(F2.mul(qx, ZZ), X)
    r2 = k2(2, F2.sub(F2.mul(qy, F2.mul(ZZ, Z)), Y))
    HH = F2.sqr(H)
    XHH = F2.mul(X, HH)
    HHH = F2.mul(HH, H)
    X3 = F2.sub(F2.sub(F2.sqr(r2), k2(4, HHH)), k2(8, XHH))
    Z3 = k2(2, F2.mul(Z, H))
    Y3 = F2.sub(F2.mul(r2, F2.sub(k2(4, XHH), X3)), k2(8, F2.mul(Y, HHH)))
    a = k2(2, Z3)
    b = F2.neg(k2(2, r2))
    c = F2.sub(k2(2, F2.mul(r2, qx)), k2(2, F2.mul(qy, Z3)))
    return X3, Y3, Z3, a, b, c


def plain2(slots):
    return (val(slots[0]) * RINV % P, val(slots[1]) * RINV % P)


def affine(X, Y, Z):
    """(X / Z^2, Y / Z^3), or None for Z = 0"""
    if F2.is_zero(Z):
        return None
    zi = F2.inv(Z)
    zi2 = F2.sqr(zi)
    return (F2.mul(X, zi2), F2.mul(Y, F2.mul(zi2, zi)))


def twist_points():
    """(points of the r-torsion, points of the twist outside it)"""
    rng = synth.SplitMix64(401)
    inside = [G2.to_affine(G2.mul(G2.to_jac(G2.gen), k)) for k in (1, 2, 3, 5, rng.field(bls.R_MOD), rng.field(bls.R_MOD))]
    outside = []
    while len(outside) < 4:
        x = (rng.field(P), rng.field(P))
        y = F2.sqrt(F2.add(F2.mul(F2.sqr(x), x), F2.b_coeff))
        if y is not None and F2.eq(F2.sqr(y), F2.add(F2.mul(F2.sqr(x), x), F2.b_coeff)):
            outside.append((x, y if len(outside) % 2 else F2.neg(y)))
    for p in inside + outside:
        assert G2.is_on_curve(p)
    assert all(G2.in_subgroup(p) for p in inside) and not any(G2.in_subgroup(p) for p in outside)
    return inside, outside


# ------------------------------------------------------------------------------------------------ cases
def build(name):
    """-> (cases, kinds): a case is the 6 / 12 input slots; kind "curve" (a point of the twist: the group law is compared too),
    "identity" (coordinates at the edges: the formulas only) or "special" (R = +-Q, Y = 0, Z = 0: only Z3 = 0 is asserted)"""
    add, quad = "ADD" in name, name.startswith("CVQ")
    zb = 4 if quad else 2                                    # the bound of Z on the way in
    L = c12.Lift(409 + OP_CODE[name])
    rng = L.rng
    inside, outside = twist_points()
    pts = inside + outside
    cases, kinds = [], []

    def l2(v, bound=2, m=None):
        return [L.comp(v[0], bound, m), L.comp(v[1], bound, m)]

    def z_slots(i):
        if i % 3 == 0:
            return [L.edge(zb), L.edge(zb)]
        if i % 3 == 1:
            return l2((rng.field(P), rng.field(P)), zb, zb - 1)
        return l2((rng.field(P), rng.field(P)), zb)

    def jac(pt, zs, m=None):
        z = plain2(zs)
        assert not F2.is_zero(z) and not F2.eq(z, F2.one)
        zz = F2.sqr(z)
        return l2(F2.mul(pt[0], zz), 2, m) + l2(F2.mul(pt[1], F2.mul(zz, z)), 2, m) + zs

    def q_slots(q, m=None):
        return l2(q[0], 2, m) + l2(q[1], 2, m) + l2(F2.sqr(q[1]), 2, m)

    def case(slots, kind):
        if add and kind == "identity":                       # y_Q^2 is what the step takes it for, in either representative
            yy = l2(F2.sqr(plain2(slots[8:10])), 2)
            slots = slots[:10] + [t if val(t) <= 2 * P - EPS else fc.exact(val(t) - P) for t in yy]
        cases.append(slots)
        kinds.append(kind)

    i = 0
    for r in pts:
        for q in (pts if add else [None] * 8):
            if add and (F2.eq(r[0], q[0])):
                continue
            i += 1
            m = (None, 1, 0)[i % 3]
            case(jac(r, z_slots(i), m) + (q_slots(q, m) if add else []), "curve")
    # every component at the edge of its bound; one component at the edge and the rest small; carries under runs of 2^28 - 1
    nq = 6 if add else 0
    for _ in range(40):
        case(L.edges(2, 4) + L.edges(zb, 2) + L.edges(2, nq), "identity")
    for s in range(6 + nq):
        case(L.one_edge(zb if s in (4, 5) else 2, s, 6 + nq), "identity")
        e = L.edges(2, 4) + L.edges(zb, 2) + L.edges(2, nq)
        e[s] = L.small(1)[0]
        case(e, "identity")
    for _ in range(12):
        case(L.runs(6 + nq), "identity")
    for _ in range(8):
        case([fc.pick(fc.operands(2), rng.below(100000)) for _ in range(4)] + [fc.pick(fc.operands(zb), rng.below(100000)) for _ in range(2)] +
             [fc.pick(fc.operands(2), rng.below(100000)) for _ in range(nq)], "identity")
    # the special cases the incomplete formulas are safe for: Z becomes 0 and stays 0
    for j, r in enumerate(pts):
        zs = z_slots(3 * j + 1)
        if add:
            case(jac(r, zs) + q_slots(r), "special")                                     # R = Q
            case(jac(r, z_slots(3 * j + 2)) + q_slots(G2.neg_affine(r)), "special")      # R = -Q
            case(l2(r[0]) + l2(r[1]) + [L.comp(0, zb, j % zb), L.comp(0, zb, (j + 1) % zb)] + q_slots(pts[(j + 1) % len(pts)]), "special")   # Z = 0
        else:
            x, z = (rng.field(P), rng.field(P)), plain2(zs)
            case(l2(x) + [L.comp(0, 2, j % 2), L.comp(0, 2, (j // 2) % 2)] + zs, "special")   # Y = 0
            case(l2(r[0]) + l2(r[1]) + [L.comp(0, zb, j % zb), L.comp(0, zb, (j + 1) % zb)], "special")                                      # Z = 0
    for c, kind in zip(cases, kinds):                        # the preconditions the header states
        c12.bounded(c[:4], 2)
        c12.bounded(c[4:6], zb)
        c12.bounded(c[6:], 2)
        assert not add or F2.eq(plain2(c[10:12]), F2.sqr(plain2(c[8:10])))
    c12.limb_forms_present(cases)
    assert any(val(s) >= zb * P - 2 * EPS for c in cases for s in c[4:6]) and any(val(s) >= 2 * P - 2 * EPS for c in cases for s in c[:4])
    # the order in which they are sent: the four rows of a wave come from distant parts of the list; the last wave is partial
    order = cc.strided(list(range(len(cases))))
    if len(order) % WAVE == 0:
        order.append(order[0])
    return [cases[i] for i in order], [kinds[i] for i in order]


def run(lib, name, cases):
    code, (_, ni) = OP_CODE[name], OPS[OP_CODE[name]]
    n = len(cases)
    assert all(len(c) == ni for c in cases) and 100 <= n <= 300, (name, n)
    a = np.zeros((n, ni, 16), dtype=np.uint32)
    for i, c in enumerate(cases):
        for s, slot in enumerate(c):
            a[i, s, :14] = slot
    a[:, :, 14:] = 0xdeadbeef          # the pad words are ignored
    out = np.full((n, 12, 16), 0xa5a5a5a5, dtype=np.uint32)
    fn = lib.dll.zk_hook_cv_step
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.check(fn(code, n, a.ctypes.data, out.ctypes.data))
    assert not out[:, :, 14:].any(), name          # pad words are zero
    return [[[int(x) for x in out[i, s, :14]] for s in range(12)] for i in range(n)]


def check_op(lib, name):
    """One hook call for the op; returns the number of cases it sent."""
    add, quad = "ADD" in name, name.startswith("CVQ")
    cases, kinds = build(name)
    out = run(lib, name, cases)
    seen = set()
    for c, o, kind in zip(cases, out, kinds):
        X, Y, Z = plain2(c[0:2]), plain2(c[2:4]), plain2(c[4:6])
        want = ref_add(X, Y, Z, plain2(c[6:8]), plain2(c[8:10])) if add else ref_double(X, Y, Z)
        got = [plain2(o[2 * t:2 * t + 2]) for t in range(6)]
        seen.add(kind)
        if kind == "special":                                # only what the header states: Z is 0 and stays 0
            assert F2.is_zero(want[2]) and F2.is_zero(got[2]), (name, kind)
            continue
        for s in range(6):                                   # the new point: weakly normalised, below 2 p (four rows: Z below 4 p)
            fc.assert_weak(o[s], (name, s))
            assert val(o[s]) < (4 if quad and s >= 4 else 2) * P, (name, s, float(fc.ratio(o[s])))
        for t, what in enumerate(("X3", "Y3", "Z3", "a", "b", "c")):
            assert got[t] == want[t], (name, kind, what)
        for s in range(6, 12):                               # the line within what k_c12_miller assumes of the stage
            fc.assert_weak(o[s], (name, s))
            assert fc.ratio(o[s]) < (64 if s >= 10 else 1000), (name, s, float(fc.ratio(o[s])))
        if kind == "curve":                                  # ... and the group law of the oracle
            r = affine(X, Y, Z)
            assert G2.is_on_curve(r)
            q = (plain2(c[6:8]), plain2(c[8:10])) if add else None
            law = G2.to_affine(G2.add(G2.to_jac(r), G2.to_jac(q)) if add else G2.dbl(G2.to_jac(r)))
            new = affine(*got[:3])
            assert law is not None and F2.eq(new[0], law[0]) and F2.eq(new[1], law[1]), (name, "group law")
    assert seen == {"curve", "identity", "special"}
    return len(cases)


def op_table_and_the_first_code_past_it(lib):
    """The ops of the C source are OPS in their order; the last code is taken and the first one past it refused without
    touching the output."""
    assert c12.ops_of_the_c_source("ZK_HK_CV_OPS", "coop_verify.cpp") == OPS
    fn = lib.dll.zk_hook_cv_step
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    a = np.zeros((1, 12, 16), dtype=np.uint32)
    out = np.full((1, 12, 16), 7, dtype=np.uint32)
    assert fn(len(OPS) - 1, 0, a.ctypes.data, out.ctypes.data) == 0
    assert fn(len(OPS), 1, a.ctypes.data, out.ctypes.data) == fc.ZK_ERR_INVALID_ARGUMENT
    assert (out == 7).all()
