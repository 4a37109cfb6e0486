"""Cases of the constraint check (zk_r1cs_check_batch, zk_transfer_check_batch, zk_anonymous_check_batch, zk_r1cs_stage) and
their reference: a_j * b_j against c_j over Python integers, row by row.  Everything a case expects comes from `reference`;
the oracle's circuits give the systems and the assignments.  Computed once per process and shared by tests/test_r1cs_check.py."""
import functools

from oracle import anonymous_circuit as ac
from oracle import bls12_381 as bls
from oracle import groth16
from oracle import synth
from oracle import transfer_circuit as tc

R = bls.R_MOD


def dot(lc, z):
    return sum(z[v] * c for v, c in lc) % R


def reference(constraints, z):
    """(the lowest j with <A_j, z> * <B_j, z> != <C_j, z> mod r, or None; how many such j; whether z_0 = 1)"""
    bad = [j for j, (a, b, c) in enumerate(constraints) if dot(a, z) * dot(b, z) % R != dot(c, z)]
    return (bad[0] if bad else None, len(bad), z[0] % R == 1)


def bad_rows(constraints, z):
    return [j for j, (a, b, c) in enumerate(constraints) if dot(a, z) * dot(b, z) % R != dot(c, z)]


class System:
    """A synthetic system and a satisfying assignment; `broken(j)`: the same system with the C side of row j off by one term's
    coefficient, which breaks row j alone for that assignment."""

    def __init__(self, name, n_in, n_aux, constraints, z):
        self.name, self.n_in, self.n_aux, self.constraints, self.z = name, n_in, n_aux, constraints, list(z)
        assert len(z) == n_in + n_aux and reference(constraints, z) == (None, 0, True), name

    def broken(self, j):
        a, b, c = self.constraints[j]
        k = next((k for k, (v, _) in enumerate(c) if self.z[v] % R), None)
        if k is None:   # c_j is zero whatever its terms hold: one more term over ONE
            c2 = list(c) + [(0, 1)]
        else:
            c2 = list(c)
            c2[k] = (c[k][0], (c[k][1] + 1) % R or 2)
        cons = list(self.constraints)
        cons[j] = (a, b, c2)
        assert bad_rows(cons, self.z) == [j]
        return cons

    def variants(self):
        """name -> assignment: satisfying; the last aux variable + 1; z_0 = 2 with everything else intact; another variable + 1"""
        last = list(self.z)
        last[-1] = (last[-1] + 1) % R
        two = list(self.z)
        two[0] = 2
        inner = list(self.z)
        inner[self.n_in] = (inner[self.n_in] + 1) % R
        return {"satisfying": self.z, "last_aux": last, "one_is_two": two, "first_aux": inner}


@functools.lru_cache(maxsize=None)
def systems():
    out = []
    chain = synth.ChainCircuit(21, 1, 1)
    inputs, aux = chain.witness(5)
    out.append(System("chain_1", 1, 1, chain.r1cs.constraints, inputs + aux))
    r1, inputs, aux = synth.random_r1cs(24, 3, 12, 20)
    out.append(System("random_20", 3, 12, r1.constraints, inputs + aux))
    # 300 rows (no multiple of 64 or 256) and, behind them: a row with an empty A (satisfied exactly when c = 0); a row of 300
    # terms between rows of one term; a row that holds only if (r - 1) * (r - 1) comes out as 1
    r1, inputs, aux = synth.random_r1cs(31, 3, 40, 300)
    z = inputs + aux
    nv = len(z)
    e_zero, e_neg, e_one, e_sum = nv, nv + 1, nv + 2, nv + 3
    long_row = [((7 * i + 1) % nv, (i * 0x9E3779B97F4A7C15 + 3) % R) for i in range(300)]
    z = z + [0, R - 1, 1, dot(long_row, z)]
    one = [(0, 1)]
    cons = list(r1.constraints) + [
        ([], [(1, 1)], [(e_zero, 1)]),
        (one, one, one),
        (long_row, one, [(e_sum, 1)]),
        (one, one, one),
        ([(e_neg, R - 1)], one, [(e_one, 1)]),
    ]
    out.append(System("random_300_plus", 3, 44, cons, z))
    return out


def to_mont(z):
    return [bls.fr_to_mont(v) for v in z]


def check_reference_against_oracle():
    """the reference above and oracle.groth16.is_satisfied say the same of a satisfying and of a broken assignment"""
    class E:   # (assign and is_satisfied read the modulus alone)
        r = R
    seen = set()
    for s in systems():
        r1 = groth16.R1CS(s.n_in, s.n_aux, s.constraints)
        for name, z in s.variants().items():
            if z[0] != 1:   # (assign refuses such an assignment outright)
                continue
            ok = groth16.is_satisfied(E, groth16.assign(E, r1, z[:s.n_in], z[s.n_in:]))
            assert ok == (reference(s.constraints, z)[1] == 0), (s.name, name)
            seen.add(ok)
    assert seen == {True, False}


# ---- the transfer circuit
@functools.lru_cache(maxsize=None)
def transfer_statement_cases():
    """(witnesses, [(first_bad, n_bad)]) of the three statements, the second with remaining_balance + 1"""
    ws = [tc.make_witness(60 + i, amount=7 + i, fee=1, balance=90 + i) for i in range(3)]
    ws[1].remaining_balance += 1
    want = []
    for w in ws:
        cs = tc.synthesize(w)
        want.append(reference(cs.to_r1cs().constraints, cs.inputs + cs.aux)[:2])
    return ws, want


@functools.lru_cache(maxsize=None)
def transfer_u32_max_case():
    """(assignment, (first_bad, n_bad)): an amount outside the range gadget"""
    cs = tc.synthesize(tc.make_witness(3, amount=0xFFFFFFFF, fee=0, balance=0xFFFFFFFF))
    z = cs.inputs + cs.aux
    return z, reference(cs.to_r1cs().constraints, z)[:2]


@functools.lru_cache(maxsize=None)
def transfer_constraints():
    return tc.synthesize(tc.make_witness(1)).to_r1cs()


# ---- the anonymous circuit
@functools.lru_cache(maxsize=None)
def anonymous_statement_cases():
    """make_witness(1), the wrong sender index and amount 11 against a remaining balance of 90 (tests/test_anonymous_circuit.py)"""
    ws = [ac.make_witness(1), ac.make_witness(1), ac.make_witness(1, amount=11)]
    ws[1].s_index = (ws[1].s_index + 1) % ac.ANONIMITY_SIZE
    if ws[1].s_index == ws[1].t_index:
        ws[1].s_index = (ws[1].s_index + 1) % ac.ANONIMITY_SIZE
    ws[2].remaining_balance = 90
    want = []
    for w in ws:
        cs = ac.synthesize(w)
        want.append(reference(cs.to_r1cs().constraints, cs.inputs + cs.aux))
    return ws, want
