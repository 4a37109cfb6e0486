"""Builders and expectations for tests/test_wallet_scan.py (zk_confidential_scan / zk_anonymous_scan).

Extrinsics are packed by hand from zk_jubjub_base_mul / zk_elgamal_encrypt / zk_elgamal_add outputs (which tests/test_gen_proof.py
and tests/test_elgamal_decrypt.py hold to the oracle) with zeroed proofs: the scan does not look at proofs.  The expectations are
computed with oracle/jubjub.py alone: the wallet's key as dk G, every used point through Point::read and [s]P == O, every value as
the logarithm of left - dk right - over a table of ALL x < limit where the limit is small, over the plaintexts a case was built
from (and their negatives) where it is 10^6 or 2^32."""
import struct

from oracle import jubjub as jj
from oracle import synth

G = jj.note_commitment_randomness_generator()
NOT_IN_FIELD, NOT_ON_CURVE, NOT_PRIME_ORDER = 1, 2, 3                      # ZK_INTO_XY_*
F_LEFT_AMOUNT_SENDER, F_LEFT_AMOUNT_RECIPIENT, F_RIGHT_RANDOMNESS, F_LEFT_FEE = 3, 4, 5, 6   # zk_confidential_verify_batch
F_LEFT_CIPHERTEXTS, F_RIGHT_CIPHERTEXT = 13, 49                            # zk_anonymous_verify_batch
SENDER, RECIPIENT = 1, 2
FOUND_SENT, FOUND_FEE, FOUND_RECEIVED = 1, 2, 4
NOT_A_POINT = bytes([0xff] * 32)                                           # y = 2^255 - 1 >= r


def fs(seed, n):
    rng = synth.SplitMix64(seed)
    return [rng.field(jj.FS_MOD) for _ in range(n)]


def neg(p):
    return ((-p[0]) % jj.R, p[1])


def torsion():
    x, y = jj.mul(G, 0x1234567)
    return jj.write_point(((-x) % jj.R, (-y) % jj.R))   # (-x, -y) = P + (0, -1): on the curve, order 2 s


def off_curve():
    y = 2
    while jj.get_for_y(y, 0) is not None:
        y += 1
    return y.to_bytes(32, "little")


WALLET, ALICE, BOB = fs(101, 3)    # decryption keys: the scanning wallet's and two strangers'
_others = {}


def other_keys(lib, count):
    """encryption keys of `count` strangers (decoys)"""
    import zero_chain_amd as zk
    if (lib.path, count) not in _others:
        _others[(lib.path, count)] = zk.jubjub_base_mul(fs(102, count), lib=lib)
    return _others[(lib.path, count)]


# ---------------------------------------------------------------------------------------------- builders
def confidential_xts(lib, specs, seed=7):
    """specs: (dec key of the sender, of the recipient, amount, fee) -> xt dicts of zero-chain_amd's XT_FIELDS, one randomness each"""
    import zero_chain_amd as zk
    n = len(specs)
    if not n:
        return []
    keys = zk.jubjub_base_mul([k for s in specs for k in s[:2]], lib=lib)
    rnd = fs(seed, n)
    vals = [v for s in specs for v in (s[2], s[2], s[3])]
    lefts, rights = zk.elgamal_encrypt(vals, [r for r in rnd for _ in range(3)], [k for i in range(n) for k in (keys[2 * i], keys[2 * i + 1], keys[2 * i])],
                                       lib=lib)
    out = []
    for i in range(n):
        out.append({"proof": bytes(192), "rsk": bytes(32), "rvk": bytes(32), "enc_balance": bytes(64), "nonce": bytes(32),
                    "enc_key_sender": keys[2 * i], "enc_key_recipient": keys[2 * i + 1], "left_amount_sender": lefts[3 * i],
                    "left_amount_recipient": lefts[3 * i + 1], "left_fee": lefts[3 * i + 2], "right_randomness": rights[3 * i]})
    return out


def anonymous_xts(lib, specs, seed=8):
    """specs: (twelve encryption keys, twelve signed values) -> xt dicts as anonymous_gen_proofs returns them.  left_i = v_i G + r key_i;
    a negative value is r key_i minus the ciphertext of |v_i| with randomness zero (zk_elgamal_add)."""
    import zero_chain_amd as zk
    n = len(specs)
    if not n:
        return []
    rnd = fs(seed, n)
    lefts, rights = zk.elgamal_encrypt([max(v, 0) for s in specs for v in s[1]], [r for r in rnd for _ in range(12)], [k for s in specs for k in s[0]],
                                       lib=lib)
    minus = [(i, j) for i, s in enumerate(specs) for j, v in enumerate(s[1]) if v < 0]
    if minus:
        la, ra = zk.elgamal_encrypt([-specs[i][1][j] for i, j in minus], [0] * len(minus), [specs[i][0][j] for i, j in minus], lib=lib)
        ls, _ = zk.elgamal_add([lefts[12 * i + j] for i, j in minus], [rights[12 * i + j] for i, j in minus], la, ra, subtract=True, lib=lib)
        for (i, j), l in zip(minus, ls):
            lefts[12 * i + j] = l
    return [{"proof": bytes(192), "nonce": bytes(32), "rsk": bytes(32), "rvk": bytes(32), "enc_keys": list(specs[i][0]),
             "left_ciphertexts": lefts[12 * i:12 * i + 12], "right_ciphertext": rights[12 * i]} for i in range(n)]


def ring(lib, wallet_key, placed):
    """twelve keys and values: `placed` maps a position to the value the wallet's key holds there, strangers with 0 elsewhere"""
    others = other_keys(lib, 12)
    return ([wallet_key if k in placed else others[k] for k in range(12)], [placed.get(k, 0) for k in range(12)])


# ---------------------------------------------------------------------------------------------- expectations
class Logs:
    """x with x G == v and x < limit: every x where the limit is small, else the candidates the case was built from"""

    def __init__(self, limit, candidates=()):
        self.limit, self.tab = limit, {}
        if limit <= 5000:
            acc = jj.ZERO
            for x in range(limit):
                self.tab[acc] = x
                acc = jj.add(acc, G)
        else:
            for c in sorted(set(abs(c) for c in candidates)):
                if c < limit:
                    self.tab[jj.mul(G, c)] = c

    def of(self, v):
        return self.tab.get(v)


def point_status(enc):
    p = jj.read_point(enc)
    if p is None:
        return NOT_IN_FIELD if int.from_bytes(enc, "little") & ((1 << 255) - 1) >= jj.R else NOT_ON_CURVE
    return 0 if jj.mul(p, jj.FS_MOD) == jj.ZERO else NOT_PRIME_ORDER


def _refusal(used):
    for field, enc in used:
        st = point_status(enc)
        if st:
            return field | st << 6
    return 0


def expected_confidential(xt, dk, logs):
    """the 16 bytes of zk_confidential_scan_result"""
    key = jj.write_point(jj.mul(G, dk))
    s, r = xt["enc_key_sender"] == key, xt["enc_key_recipient"] == key
    role = (SENDER if s else 0) | (RECIPIENT if r else 0)
    if not role:
        return bytes(16)
    used = ([(F_LEFT_AMOUNT_SENDER, xt["left_amount_sender"])] if s else []) + ([(F_LEFT_AMOUNT_RECIPIENT, xt["left_amount_recipient"])] if r else []) + \
           [(F_RIGHT_RANDOMNESS, xt["right_randomness"])] + ([(F_LEFT_FEE, xt["left_fee"])] if s else [])
    refusal = _refusal(used)
    found, vals = 0, [0, 0, 0]
    if not refusal:
        minus = neg(jj.mul(jj.read_point(xt["right_randomness"]), dk))
        for k, (on, bit, name) in enumerate(((s, FOUND_SENT, "left_amount_sender"), (s, FOUND_FEE, "left_fee"), (r, FOUND_RECEIVED, "left_amount_recipient"))):
            x = logs.of(jj.add(jj.read_point(xt[name]), minus)) if on else None
            if x is not None:
                found |= bit
                vals[k] = x
    return struct.pack("<BBBBIII", role, found, refusal, 0, *vals)


def expected_anonymous(xt, dk, logs):
    """the 16 bytes of zk_anonymous_scan_result"""
    key = jj.write_point(jj.mul(G, dk))
    where = [k for k in range(12) if xt["enc_keys"][k] == key]
    if not where:
        return bytes(16)
    members = sum(1 << k for k in where)
    refusal = _refusal([(F_LEFT_CIPHERTEXTS + k, xt["left_ciphertexts"][k]) for k in where] + [(F_RIGHT_CIPHERTEXT, xt["right_ciphertext"])])
    found, delta = 0, 0
    if not refusal:
        minus = neg(jj.mul(jj.read_point(xt["right_ciphertext"]), dk))
        vals = []
        for k in where:
            v = jj.add(jj.read_point(xt["left_ciphertexts"][k]), minus)
            plus, less = logs.of(v), logs.of(neg(v))
            vals.append(plus if plus is not None else None if less is None else -less)
        if all(v is not None for v in vals):
            found, delta = 1, sum(vals)
    return struct.pack("<HBBIq", members, found, refusal, 0, delta)


# ---------------------------------------------------------------------------------------------- the cases
def confidential_role_cases(lib, amounts, fee_over, limit):
    """sender, recipient, a transfer to oneself for every amount; neither; a fee of 0 and one above the limit; a ciphertext under a
    stranger's key in an xt whose enc_key_recipient is the wallet's.  Returns (xts, candidates)."""
    import zero_chain_amd as zk
    specs = []
    for a in amounts:
        specs += [(WALLET, ALICE, a, 3), (ALICE, WALLET, a, 3), (WALLET, WALLET, a, 1)]
    specs += [(ALICE, BOB, 9, 3), (WALLET, ALICE, 7, 0), (WALLET, BOB, 7, fee_over), (ALICE, WALLET, 11, 2)]
    xts = confidential_xts(lib, specs)
    (bob_key,) = zk.jubjub_base_mul([BOB], lib=lib)
    (l,), _ = zk.elgamal_encrypt([11], fs(7, len(specs))[-1:], [bob_key], lib=lib)   # the last xt's randomness, Bob's key
    xts[-1]["left_amount_recipient"] = l
    return xts, list(amounts) + [0, 1, 2, 3, 7, 9, 11, fee_over]


def anonymous_cases(lib, amounts, over, limit_is_one=False):
    """absent, decoy, recipient and sender for every amount, |a| = over (not found), positions 0 and 11, twice in one ring (recipient
    and decoy; +300 and -7; one occurrence above the limit).  Returns (xts, candidates)."""
    import zero_chain_amd as zk
    (w,) = zk.jubjub_base_mul([WALLET], lib=lib)
    specs = [ring(lib, w, {}), ring(lib, w, {5: 0})]
    for i, a in enumerate(amounts):
        specs += [ring(lib, w, {(3 * i) % 12: a}), ring(lib, w, {(3 * i + 1) % 12: -a})]
    specs += [ring(lib, w, {2: over}), ring(lib, w, {2: -over}), ring(lib, w, {0: amounts[0]}), ring(lib, w, {11: -amounts[-1]}),
              ring(lib, w, {4: amounts[1], 9: 0}), ring(lib, w, {1: 300, 10: -7}), ring(lib, w, {0: 5, 11: -over}), ring(lib, w, {3: over, 6: 0})]
    return anonymous_xts(lib, specs), list(amounts) + [0, 5, 7, 300, over]


def refusal_cases(lib):
    """(confidential xts, anonymous xts): bad points in matching extrinsics between good ones, then the same bad points in extrinsics
    that do not match"""
    import zero_chain_amd as zk
    (w,) = zk.jubjub_base_mul([WALLET], lib=lib)
    t, off = torsion(), off_curve()
    good = [(ALICE, WALLET, 40, 1), (WALLET, ALICE, 41, 2), (WALLET, WALLET, 42, 3)]
    cx = confidential_xts(lib, good + [good[0], good[1], good[1], good[2], good[0], (ALICE, BOB, 5, 1), (ALICE, BOB, 5, 1)] + good)
    cx[3]["left_amount_recipient"] = t               # recipient: field 4, not of prime order
    cx[4]["right_randomness"] = NOT_A_POINT          # sender: field 5, not in the field
    cx[5]["left_fee"] = off                          # sender: field 6, not on the curve (3 and 5 are fine)
    cx[6].update(left_amount_sender=NOT_A_POINT, left_amount_recipient=t)   # both roles: the first in push order, field 3
    cx[7].update(left_amount_sender=t, left_fee=NOT_A_POINT)                # recipient only: the sender's points are not looked at
    cx[8].update(left_amount_recipient=t, right_randomness=NOT_A_POINT)     # no match: nothing is looked at
    cx[9].update(left_amount_sender=off, left_fee=t)
    ax = anonymous_xts(lib, [ring(lib, w, {3: 17}), ring(lib, w, {6: -9}), ring(lib, w, {2: 5, 7: 0}), ring(lib, w, {1: 1}), ring(lib, w, {}),
                             ring(lib, w, {}), ring(lib, w, {0: 17})])
    ax[1]["left_ciphertexts"][6] = t                 # field 19, not of prime order
    ax[2]["left_ciphertexts"][7] = NOT_A_POINT       # the second occurrence: field 20
    ax[2]["left_ciphertexts"][3] = t                 # (a stranger's ciphertext: not looked at)
    ax[3]["right_ciphertext"] = off                  # field 49
    ax[4]["left_ciphertexts"][0] = t                 # no match
    ax[5]["right_ciphertext"] = NOT_A_POINT
    return cx, ax, [1, 2, 3, 5, 9, 17, 40, 41, 42]


def lane_layout_cases(lib):
    """23 transfers to oneself (92 points: kind 1 ends inside its second wave; 23 rights from lane 128; 69 rows); the same with a
    stranger's transfer between every two; one call whose only match is its last extrinsic"""
    own = [(WALLET, WALLET, 100 + 7 * i, i) for i in range(23)]
    mixed = [s for o in own for s in (o, (ALICE, BOB, 1, 1))][:-1]
    last = [(ALICE, BOB, 2, 1)] * 5 + [(BOB, WALLET, 77, 1)]
    cand = [100 + 7 * i for i in range(23)] + list(range(23)) + [77]
    return confidential_xts(lib, own), confidential_xts(lib, mixed), confidential_xts(lib, last), cand
