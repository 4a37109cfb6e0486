"""Requests for zk_anonymous_derive_dev (tests/test_anon_derive.py) and the Python model of what it writes.

A request is the dict zk.anonymous_requests takes.  Its points come from a pool of prime-order encodings ([k]G for fixed scalars k,
computed once by the oracle), so that building a batch costs no multiplication; the balances need not be consistent with
anything, since the derivation only decodes them.  The model is oracle.gen_proof.gen_anonymous_xt_fields - the restatement of
anonymous.rs:97-183 that tests/test_gen_proof.py checks zk_anonymous_derive against - with the 104 public inputs of check_proof
(anonymous.rs:213-264) read off the points it returns.  It costs 13 multiplications and is computed once per distinct request."""
from oracle import anonymous_circuit as ac
from oracle import gen_proof as og
from oracle import jubjub as jj
from oracle import synth

import scan_cases as sc

G = jj.note_commitment_randomness_generator()
IDENTITY = jj.write_point(jj.ZERO)
SMALL_ORDER = (jj.R - 1).to_bytes(32, "little")                       # (0, -1): on the curve, of order 2
BAD_ENCODINGS = (("y not in the field", sc.NOT_A_POINT, "is not a Jubjub point"),
                 ("off the curve", sc.off_curve(), "is not a Jubjub point"),
                 ("small order", SMALL_ORDER, "is not in the prime-order subgroup"),
                 ("torsion", sc.torsion(), "is not in the prime-order subgroup"))
POOL_SIZE = 96
_pool = []


def pool():
    """POOL_SIZE prime-order encodings, [k]G by repeated addition of a random multiple of G"""
    if not _pool:
        step = jj.mul(G, sc.fs(907, 1)[0])
        p = jj.mul(G, 0x1f2e3d4c5b6a7988)
        for _ in range(POOL_SIZE):
            p = jj.add(p, step)
            _pool.append(jj.write_point(p))
    return _pool


def sender_key(seed):
    return og.spending_key_from_seed(b"anon derive sender %d" % seed)


def request(seed, amount=10, balance=100, s_index=None, t_index=None, first=None, **over):
    """Request `seed`: its points are pool entries from `first` on (default: a window of its own per seed, so that two
    requests with different seeds below 2 share nothing; pass the same `first` to share all), everything else from a generator
    seeded with `seed`; `over` replaces fields."""
    rng = synth.SplitMix64(1000 + seed)
    P = pool()
    at = (36 * seed if first is None else first)
    take = lambda k: P[(at + k) % POOL_SIZE]
    s = rng.below(12) if s_index is None else s_index
    t = (s + 1 + rng.below(11)) % 12 if t_index is None else t_index
    rq = dict(amount=amount, remaining_balance=balance - amount, s_index=s, t_index=t, spending_key=sender_key(seed),
              enc_key_recipient=take(0), enc_keys_decoy=[take(1 + j) for j in range(10)], g_epoch=take(11),
              enc_balances_left=[take(12 + 2 * i) for i in range(12)], enc_balances_right=[take(13 + 2 * i) for i in range(12)],
              randomness=rng.field(jj.FS_MOD), alpha=rng.field(jj.FS_MOD))
    rq.update(over)
    return rq


def _key(rq):
    return repr(sorted((k, v) for k, v in rq.items()))


_model = {}


def expected(rq):
    """(statement dict as anonymous_circuit.statement_dict's, rsk bytes, the 104 public inputs as ints) of a valid request"""
    k = _key(rq)
    if k not in _model:
        rd = jj.read_point
        bals = [(rd(l), rd(r)) for l, r in zip(rq["enc_balances_left"], rq["enc_balances_right"])]
        g_epoch = rd(rq["g_epoch"])
        fields, stmt = og.gen_anonymous_xt_fields(rq["spending_key"], rq["amount"], rq["remaining_balance"], rq["s_index"], rq["t_index"],
                                                  rd(rq["enc_key_recipient"]), [rd(d) for d in rq["enc_keys_decoy"]], bals, g_epoch,
                                                  rq["randomness"], rq["alpha"])
        d = ac.statement_dict(stmt)
        # the balances and g_epoch pass through as the bytes that came (an encoding need not be the canonical one)
        d["enc_balances_left"], d["enc_balances_right"], d["g_epoch"] = list(rq["enc_balances_left"]), list(rq["enc_balances_right"]), rq["g_epoch"]
        pts = [rd(e) for e in fields["enc_keys"]] + [rd(e) for e in fields["left_ciphertexts"]] + [b[0] for b in bals] + [b[1] for b in bals]
        pts += [rd(fields["right_ciphertext"]), rd(fields["rvk"]), g_epoch, rd(fields["nonce"])]
        _model[k] = (d, fields["rsk"], [c for p in pts for c in p], fields)
    return _model[k]


def statement_dict(st):
    """a zk_anonymous_statement of the library in the shape of anonymous_circuit.statement_dict"""
    d = {n: int(getattr(st, n)) for n in ("amount", "remaining_balance", "s_index", "t_index")}
    for n in ("randomness", "alpha", "dec_key"):
        d[n] = int.from_bytes(bytes(getattr(st, n)), "little")
    for n in ("proof_generation_key", "g_epoch"):
        d[n] = bytes(getattr(st, n))
    for n in ("enc_keys", "left_ciphertexts", "enc_balances_left", "enc_balances_right"):
        d[n] = [bytes(e) for e in getattr(st, n)]
    return d


# the fields of a request in the order both forms decode them, with a way to replace each
def field_kinds():
    """(name in the message, function(rq, encoding) -> the request with that field replaced), one per KIND of field at a position
    of its own: the recipient, a first / middle / last decoy, g_epoch, balance halves of the first and last member"""
    def decoy(j):
        return lambda rq, e: dict(rq, enc_keys_decoy=rq["enc_keys_decoy"][:j] + [e] + rq["enc_keys_decoy"][j + 1:])

    def bal(side, i):
        return lambda rq, e: dict(rq, **{side: rq[side][:i] + [e] + rq[side][i + 1:]})
    return [("enc_key_recipient", lambda rq, e: dict(rq, enc_key_recipient=e)),
            ("enc_keys_decoy[0]", decoy(0)), ("enc_keys_decoy[9]", decoy(9)),
            ("g_epoch", lambda rq, e: dict(rq, g_epoch=e)),
            ("enc_balances_left[0]", bal("enc_balances_left", 0)), ("enc_balances_right[11]", bal("enc_balances_right", 11)),
            ("enc_balances_right[4]", bal("enc_balances_right", 4))]
