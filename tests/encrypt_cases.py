"""Inputs for zk_elgamal_encrypt_dev (tests/test_elgamal_encrypt_dev.py) and the Python model of what it writes.

A call is (values, randomness, enc_keys, k): len(randomness) groups of k keys, values and keys flat, group after group.  The keys
come from a pool of prime-order encodings ([j]G by repeated addition, computed once by the oracle), so that building a call costs
no multiplication.  The model is oracle.jubjub on integers - left = v G + r pk, right = r G, written as Point::write, and the
status of a key as Point::read and [s]P == O decide it (scan_cases.point_status) - computed once per distinct (key, r) and per
distinct value.  The refused encodings are the ones scan_cases / anon_derive_cases already provide."""
from oracle import jubjub as jj
from oracle import synth

import scan_cases as sc

G = sc.G
S = jj.FS_MOD
IDENTITY = jj.write_point(jj.ZERO)
ZERO_BYTES = bytes(32)
TOP = (1 << 32) - 1
POOL_SIZE = 64
_pool, _points, _status, _var, _fixed = [], {}, {}, {}, {}


def pool():
    """POOL_SIZE prime-order encodings"""
    if not _pool:
        step = jj.mul(G, sc.fs(911, 1)[0])
        p = jj.mul(G, 0x2b7e151628aed2a6)
        for _ in range(POOL_SIZE):
            p = jj.add(p, step)
            _pool.append(jj.write_point(p))
            _points[_pool[-1]] = p
            _status[_pool[-1]] = 0
    return _pool


def keys(first, count):
    P = pool()
    return [P[(first + j) % POOL_SIZE] for j in range(count)]


def randomness(seed, count):
    return sc.fs(5000 + seed, count)


def status(enc):
    if enc not in _status:
        _status[enc] = sc.point_status(enc)
    return _status[enc]


def _point(enc):
    if enc not in _points:
        _points[enc] = jj.read_point(enc)
    return _points[enc]


def base_mul(v):
    """[v]G for any integer v, negative ones as the negated point"""
    if abs(v) not in _fixed:
        _fixed[abs(v)] = jj.mul(G, abs(v))
    return sc.neg(_fixed[abs(v)]) if v < 0 else _fixed[abs(v)]


def expected_left(v, r, enc):
    """(bytes, status) of one left ciphertext"""
    st = status(enc)
    if st:
        return ZERO_BYTES, st
    if (enc, r) not in _var:
        _var[(enc, r)] = jj.mul(_point(enc), r)
    return jj.write_point(jj.add(base_mul(v), _var[(enc, r)])), 0


def expected_right(r):
    return jj.write_point(base_mul(r))


def expected_group(values, rnd, enc_keys, k, i):
    """(lefts, right, statuses) of group i of a call"""
    pairs = [expected_left(values[i * k + j], rnd[i], enc_keys[i * k + j]) for j in range(k)]
    return [p[0] for p in pairs], expected_right(rnd[i]), [p[1] for p in pairs]


def confidential(seed, n):
    """n groups of k = 3: (amount, amount, fee) under (sender, recipient, sender) - MultiCiphertexts::<Confidential>::encrypt"""
    rng = synth.SplitMix64(7000 + seed)
    values, enc = [], []
    for i in range(n):
        sender, recipient = keys(2 * i + seed, 2)
        amount, fee = 1 + rng.below(1 << 20), 1 + rng.below(100)
        values += [amount, amount, fee]
        enc += [sender, recipient, sender]
    return values, randomness(seed, n), enc, 3


def anonymous(seed, n, first=0, shared=False):
    """n groups of k = 12: -a at the sender, +a at the recipient, ten zeros - MultiCiphertexts::<Anonymous>::encrypt; with `shared`
    every group has the same ring"""
    rng = synth.SplitMix64(8000 + seed)
    values, enc = [], []
    for i in range(n):
        s = rng.below(12)
        t = (s + 1 + rng.below(11)) % 12
        a = 1 + rng.below(1 << 20)
        values += [-a if j == s else a if j == t else 0 for j in range(12)]
        enc += keys(first if shared else first + 12 * i, 12)
    return values, randomness(seed, n), enc, 12
