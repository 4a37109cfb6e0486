"""Builders and expectations for tests/test_balance_keys.py (zk_balance_keys).

Accounts are the dicts the block executors take and return; their ciphertexts come from the product's zk_elgamal_encrypt (which
tests/test_gen_proof.py holds to the oracle).  The expectations are computed with oracle/jubjub.py alone, on the encodings: the hit
is the account whose enc_key is dk G for a key of the set, every USED point goes through Point::read and [s]P == O in the order
balance left, balance right, pending left, pending right, the total is the sum of the used halves, enc_total Point::write of both,
and the value the logarithm of L - dk R over scan_cases.Logs."""
import struct

import scan_cases as sc
import scan_keys_cases as skc
from oracle import jubjub as jj

DUE = 1                                              # ZK_BLOCK_ROLLOVER_DUE
IDENTITY = b"\x01" + bytes(31)
ZERO_CT = (IDENTITY, IDENTITY)                       # Ciphertext::zero()
HIT = struct.Struct("<IIBBBBI64s")                   # zk_balance_hit: account, key, found, refusal, pending_added, reserved, value, enc_total
assert HIT.size == 80


def accounts(lib, specs, seed):
    """specs: (decryption key, balance, pending, flags), a value being an int or None for Ciphertext::zero() -> account dicts"""
    import zero_chain_amd as zk
    keys = zk.jubjub_base_mul([s[0] for s in specs], lib=lib)
    slots = [(i, f) for i, s in enumerate(specs) for f in (1, 2) if s[f] is not None]
    rnd = sc.fs(seed, len(slots))
    lefts, rights = zk.elgamal_encrypt([specs[i][f] for i, f in slots], rnd, [keys[i] for i, _ in slots], lib=lib) if slots else ([], [])
    ct = dict(zip(slots, zip(lefts, rights)))
    return [{"enc_key": keys[i], "balance": ct.get((i, 1), ZERO_CT), "pending": ct.get((i, 2), ZERO_CT), "flags": s[3]} for i, s in enumerate(specs)]


def with_flags(accs, flags):
    return [dict(a, flags=f) for a, f in zip(accs, flags)]


_status, _product = {}, {}


def status(enc):
    if enc not in _status:
        _status[enc] = sc.point_status(enc)
    return _status[enc]


def expected_hits(accs, dks, logs):
    """[80 bytes] of the hits for the key set `dks`, in account order, by the oracle alone"""
    enc = {jj.write_point(jj.mul(sc.G, dk)): k for k, dk in enumerate(dks)}
    out = []
    for i, a in enumerate(accs):
        k = enc.get(a["enc_key"])
        if k is None:
            continue
        due = a["flags"] & DUE
        used = [a["balance"][0], a["balance"][1]] + ([a["pending"][0], a["pending"][1]] if due else [])
        refusal = next((f + 1 | status(e) << 6 for f, e in enumerate(used) if status(e)), 0)
        if refusal:
            out.append(HIT.pack(i, k, 0, refusal, due, 0, 0, bytes(64)))
            continue
        pts = [jj.read_point(e) for e in used]
        left, right = (jj.add(pts[0], pts[2]), jj.add(pts[1], pts[3])) if due else (pts[0], pts[1])
        memo = (jj.write_point(right), dks[k])
        if memo not in _product:
            _product[memo] = jj.mul(right, dks[k])
        x = logs.of(jj.add(left, sc.neg(_product[memo])))
        out.append(HIT.pack(i, k, x is not None, 0, due, 0, x or 0, jj.write_point(left) + jj.write_point(right)))
    return out


def plain_hit(account, key, balance, pending, flags, limit, enc_total):
    """the 80 bytes from the plaintexts an account was built from (the random set: the oracle holds the small cases)"""
    total = (balance or 0) + ((pending or 0) if flags & DUE else 0)
    found = total < limit
    return HIT.pack(account, key, found, 0, flags & DUE, 0, total if found else 0, enc_total)


# ---------------------------------------------------------------------------------------------- the cases
def value_cases(lib, values, over):
    """WALLET's accounts, due: every value as the balance with itself and with the value three further on as the pending (where the
    sum stays a u32), the largest beside a zero on either side; then a sum that reaches `over` only with the pending, due and with
    the bit clear.  Returns (accounts, candidates)."""
    n = len(values)
    pairs = [(values[i], values[(i + k) % n]) for i in range(n) for k in (0, 3)] + [(values[-1], 0), (0, values[-1])]
    specs = [(sc.WALLET, b, p, DUE) for b, p in pairs if b + p < 1 << 32]
    specs += [(sc.WALLET, over - 1, 1, DUE), (sc.WALLET, over - 1, 1, 0)]
    return accounts(lib, specs, 41), sorted(set(b + p for _, b, p, _ in specs) | set(values))


def zero_cases(lib):
    """Ciphertext::zero() as pending, as balance, as both - due and not"""
    specs = [(sc.WALLET, 7, None, DUE), (sc.ALICE, None, 9, DUE), (sc.BOB, None, None, DUE), (sc.WALLET, None, 9, 0), (sc.ALICE, None, None, 0)]
    return accounts(lib, specs, 42), [0, 7, 9]


def edge_cases(lib, values):
    """the five keys of scan_keys_cases.EDGE, each owning one due account"""
    return accounts(lib, [(dk, values[j], j + 1, DUE) for j, dk in enumerate(skc.EDGE)], 43), [values[j] + j + 1 for j in range(5)]


def lane_layout_cases(lib):
    """65 due accounts over the keys of CYCLE: 260 point lanes and 130 multiplication lanes, the last wave of every kind partial;
    the same with every second account not due (97 multiplication lanes, rows no longer 2h, 2h + 1); that one with a stranger's
    account between every two; accounts whose only hit is the last.  Returns (due, mixed, strangers, last, candidates)."""
    specs = [(skc.CYCLE[j % 5], 100 + 7 * j, 1 + j % 9, DUE) for j in range(65)]
    due = accounts(lib, specs, 44)
    mixed = with_flags(due, [DUE if j % 2 == 0 else 0 for j in range(65)])
    other = accounts(lib, [(skc.STRANGERS[j % 3], 5, 6, DUE) for j in range(64)], 45)
    strangers = [a for pair in zip(mixed, other + [None]) for a in pair][:-1]
    last = other[:5] + [due[3]]
    return due, mixed, strangers, last, [100 + 7 * j for j in range(65)] + [101 + 7 * j + j % 9 for j in range(65)]


def asset_cases(lib):
    """the asset shape: three accounts under one key (one per asset id), between two of another key"""
    specs = [(sc.ALICE, 1, 2, DUE), (sc.WALLET, 10, 1, DUE), (sc.WALLET, 20, 2, 0), (sc.ALICE, 3, 4, 0), (sc.WALLET, 30, 3, DUE)]
    return accounts(lib, specs, 46), [3, 11, 20, 33]


def refusal_cases(lib):
    """WALLET's and ALICE's good accounts around: each of the four fields in turn refused in each of the three ways (due accounts);
    two bad fields in one account; a bad pending on an account that is not due; bad points in a stranger's account.  Returns
    (accounts, candidates, {account index: expected refusal byte})."""
    bad = [sc.NOT_A_POINT, sc.off_curve(), sc.torsion()]
    good = [(sc.WALLET, 40, 2, DUE), (sc.ALICE, 41, 3, DUE)]
    accs = accounts(lib, [good[0]] + [(sc.WALLET if j % 2 else sc.ALICE, 50 + j, 1, DUE) for j in range(12)] + [good[1], (sc.WALLET, 60, 1, DUE), (sc.ALICE, 61, 1, 0),
                                                                                                               (skc.STRANGERS[0], 62, 1, DUE), good[0]], 47)
    want = {}

    def spoil(a, field, way):
        name, half = ("balance", "pending")[(field - 1) >> 1], (field - 1) & 1
        c = list(a[name])
        c[half] = bad[way]
        a[name] = tuple(c)
    for field in range(1, 5):
        for way in range(3):
            i = 1 + 3 * (field - 1) + way
            spoil(accs[i], field, way)
            want[i] = field | (way + 1) << 6
    spoil(accs[14], 4, 0)          # two bad points: the first in the order of the fields
    spoil(accs[14], 2, 2)
    want[14] = 2 | 3 << 6
    spoil(accs[15], 3, 1)          # not due: the pending is not read
    spoil(accs[15], 4, 0)
    spoil(accs[16], 1, 0)          # a stranger's: not looked at
    spoil(accs[16], 2, 2)
    assert len(accs) == 18 and sc.point_status(bad[1]) == sc.NOT_ON_CURVE and sc.point_status(bad[2]) == sc.NOT_PRIME_ORDER
    return accs, [42, 44, 61], want
