"""The cases of tests/test_ntt_passes.py: the Fr transform (csrc/ntt.h k_ntt_pass), its planner (csrc/ntt_plan.h) and the tables
of NttPlan::init (csrc/zkamd.cpp), through the test hooks zk_hook_ntt_plan / zk_hook_ntt_chain / zk_hook_ntt_table and the public
zk_ntt_run_dev.  Every function takes `lib` (a ZkLib over the emulation build or over libzkamd_hooks.so).

The reference is Python integers: dif_stage / dit_stage apply ONE butterfly stage to a list mod r by the textbook definition.
The transform is linear and the twiddle tables hold Montgomery forms, so mul(v, tw[e]) = v w^e on the residues as they are: the
test chooses the residues (the limbs the kernel's add and sub see) and expects the reference applied to those residues with the
plain values of the twiddles.  From 2^14 on the whole chain is compared with the C restatement of bellman's fft (oracle/cport.py)
on the same bytes - the same linearity - with the bit reversal applied in numpy.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np

from oracle import bls12_381 as bls
from oracle import cport

R = bls.R_MOD
MONT = bls.FR_R                      # 2^256 mod r
MONT_INV = pow(MONT, -1, R)
GEN = bls.FR_GENERATOR
ZK_ERR_INVALID_ARGUMENT = 16
ZK_BAD_SCALAR = 1
LATENCY, SMALL, MID, BIG, AUTO = 0, 1, 2, 3, -1
FORM_NAMES = {LATENCY: "latency", SMALL: "small", MID: "mid", BIG: "big"}
TABLES = ("tw_fwd", "tw_inv", "s1_plain", "s1_mont", "s2", "dt", "sc_plain", "sc_mont", "coset_fwd", "coset_inv", "consts")
SENTINEL = 0xA5A5A5A5                # every word of a gap element: a value >= r that no kernel may read or write
GAP = 5


def omega(k):
    """the 2^k-th root of unity of the domain (domain.rs: ROOT_OF_UNITY squared S - k times)"""
    return pow(bls.FR_ROOT_OF_UNITY, 1 << (bls.FR_S - k), R)


@functools.lru_cache(maxsize=None)
def twiddles(k, inverse):
    """w^e (or w^-e) for e < n / 2, as an object array"""
    w = omega(k)
    if inverse:
        w = pow(w, -1, R)
    out, x = [], 1
    for _ in range((1 << k) >> 1):
        out.append(x)
        x = x * w % R
    return np.array(out, dtype=object)


def bitrev(i, k):
    return int(bin(i)[2:].zfill(k)[::-1], 2) if k else 0


@functools.lru_cache(maxsize=None)
def bitrev_perm(k):
    n = 1 << k
    i = np.arange(n, dtype=np.int64)
    r = np.zeros(n, dtype=np.int64)
    for b in range(k):
        r |= ((i >> b) & 1) << (k - 1 - b)
    return r


# ------------------------------------------------------------------------------------------------ the reference: one stage
def dif_stage(v, k, t, inverse=False):
    """DIF stage t of a 2^k-point transform, distance d = n >> (t + 1): for every i with bit d clear,
    u = x + y, v = (x - y) w^((i mod d) << t) with x = v[i], y = v[i + d]."""
    n = 1 << k
    d = n >> (t + 1)
    tw = twiddles(k, inverse)
    a = np.array(v, dtype=object).reshape(n // (2 * d), 2, d)      # [block][upper | lower][i mod d]
    x, y = a[:, 0, :], a[:, 1, :]
    w = tw[np.arange(d) << t]
    out = np.empty_like(a)
    out[:, 0, :] = (x + y) % R
    out[:, 1, :] = (x - y) * w % R
    return list(out.reshape(n))


def dit_stage(v, k, j, inverse=False):
    """DIT stage j, distance d = 2^j: y' = y w^((i mod d) << (k - 1 - j)), then x + y', x - y'."""
    n = 1 << k
    d = 1 << j
    tw = twiddles(k, inverse)
    a = np.array(v, dtype=object).reshape(n // (2 * d), 2, d)
    x, y = a[:, 0, :], a[:, 1, :] * tw[np.arange(d) << (k - 1 - j)] % R
    out = np.empty_like(a)
    out[:, 0, :] = (x + y) % R
    out[:, 1, :] = (x - y) % R
    return list(out.reshape(n))


def stages(v, k, dif, inverse, t0, g):
    for t in range(t0, t0 + g):
        v = dif_stage(v, k, t, inverse) if dif else dit_stage(v, k, t, inverse)
    return v


# ------------------------------------------------------------------------------------------------ bytes
def pack(vals):
    """integers -> (len, 8) uint32 words, little-endian limbs"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), dtype=np.uint32).reshape(-1, 8).copy()


def unpack(words):
    b = np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def random_residues(seed, count):
    """numpy's bytes with the top byte below 0x73: residues below r (whose top byte is 0x73)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] = rng.integers(0, 0x73, size=count, dtype=np.uint8)
    return a.view(np.uint32).reshape(count, 8)


def c_fft(words, k, dif, inverse):
    """What a whole chain makes of the residues `words` ((n, 8) uint32), from bellman's fft in C on the same bytes.  A DIF chain
    takes natural order to bit-reversed order, a DIT chain the other way; the inverse twiddles give the forward transform of
    the sequence read backwards (x[-i mod n]), without the 1 / n."""
    n = 1 << k
    br = bitrev_perm(k)
    x = words if dif else words[br]
    if inverse:
        x = x[(-np.arange(n)) % n]
    out = np.frombuffer(cport.fft(np.ascontiguousarray(x).tobytes(), k, False, False, 4), dtype=np.uint32).reshape(n, 8)
    return out[br] if dif else out


# ------------------------------------------------------------------------------------------------ the hooks
def plan(lib, k, batch, dif, form):
    """(form chosen, [(t0, g, log_cw, dif, threads, grid_x, lds_bytes)]) or the status of a refusal"""
    fn = lib.dll.zk_hook_ntt_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    words = np.full(1 + 7 * 32, 0xffffffff, dtype=np.uint32)
    nw = C.c_size_t(0)
    st = fn(k, batch, int(dif), form, words.ctypes.data, words.size, C.byref(nw))
    if st != 0:
        return st
    assert (nw.value - 1) % 7 == 0
    return int(words[0]), [tuple(int(x) for x in words[1 + 7 * i:8 + 7 * i]) for i in range((nw.value - 1) // 7)]


def chain(lib, k, form, dif, inverse, data, stride, pre=None, post=None, src=None, src_stride=0, src_valid=0, minus=None,
          minus_stride=0, first=0, count=0xffffffff, status=False):
    """NttPlan::chain on `data` ((batch * stride, 8) uint32, changed in place); returns the flag word (or the status)."""
    fn = lib.dll.zk_hook_ntt_chain
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    n = 1 << k
    assert data.dtype == np.uint32 and data.flags.c_contiguous and data.shape[0] % stride == 0
    batch = data.shape[0] // stride
    for tab in (pre, post):
        assert tab is None or (tab.shape == (n, 8) and tab.dtype == np.uint32 and tab.flags.c_contiguous)
    assert src is None or (src.shape == (batch * src_stride, 8) and src.dtype == np.uint32 and src.flags.c_contiguous)
    assert minus is None or (minus.shape == (batch * minus_stride, 8) and minus.dtype == np.uint32 and minus.flags.c_contiguous)
    ptr = lambda a: None if a is None else a.ctypes.data
    bad = C.c_uint32(0xffffffff)
    st = fn(k, form, int(dif), int(inverse), batch, stride, data.ctypes.data, ptr(pre), ptr(post), ptr(src), src_stride, src_valid,
            ptr(minus), minus_stride, first, count, C.byref(bad))
    if status:
        return st
    lib.check(st)
    return bad.value


def table(lib, k, which):
    fn = lib.dll.zk_hook_ntt_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    nb = C.c_size_t(0)
    lib.check(fn(k, TABLES.index(which), None, 0, C.byref(nb)))
    out = np.zeros(nb.value // 4 + 8, dtype=np.uint32)
    lib.check(fn(k, TABLES.index(which), out.ctypes.data, nb.value, C.byref(nb)))
    assert nb.value % 32 == 0
    return unpack(out[:nb.value // 4])


# ------------------------------------------------------------------------------------------------ a. the plan
def check_plan_invariants(lib):
    """every form at every size it is allowed for: the passes cover the k stages once, tile the n elements once, fit the LDS and
    the block; returns the number of plans looked at"""
    seen = 0
    for form in (LATENCY, SMALL, MID, BIG):
        for k in range(0, 28):
            for dif in (1, 0):
                got = plan(lib, k, 1, dif, form)
                if form == MID and k < 11:
                    assert got == ZK_ERR_INVALID_ARGUMENT, (form, k)
                    continue
                chosen, ps = got
                assert chosen == form
                if k == 0:
                    assert ps == []
                    continue
                seen += 1
                t = 0
                for (t0, g, lcw, d, threads, grid_x, lds) in ps:
                    what = (FORM_NAMES[form], k, dif, t0)
                    assert t0 == t and g >= 1 and d == dif, what
                    t += g
                    assert lcw <= k - g, what
                    assert grid_x >= 1 and grid_x << (g + lcw) == 1 << k, what
                    assert lds == 32 << (g + lcw) and lds <= 160 * 1024, what
                    assert 1 <= threads <= 1024, what
                    if form == LATENCY:
                        # one butterfly per thread and stage is what this form is: nothing in the kernel's loops needs it
                        assert threads == (1 << (g + lcw)) >> 1 and g + lcw <= 8, what
                    else:
                        assert threads == {SMALL: 256, MID: 512, BIG: 1024}[form], what
                        assert g <= {SMALL: 8, MID: 11, BIG: 10}[form] and g + lcw <= {SMALL: 10, MID: 11, BIG: 12}[form], what
                assert t == k, (FORM_NAMES[form], k, dif)
    for bad_form in (4, 5, 0x10, 0x14, -2):
        assert plan(lib, 12, 1, 1, bad_form) == ZK_ERR_INVALID_ARGUMENT
    assert plan(lib, 28, 1, 1, SMALL) == ZK_ERR_INVALID_ARGUMENT
    return seen


# ------------------------------------------------------------------------------------------------ b. pass by pass
KINDS = ("random", "zero", "r-1", "equal", "sum=r", "sum=r-1", "sum=r+1", "one@0", "one@1", "one@n/2", "one@n-1", "random2")


def _partner_inputs(kind, k, dif, inverse, t, seed):
    """x random, and y at the partner of the pass's first stage `t` so that the two operands of that stage's add / sub - x and y
    for DIF, x and y w^e for DIT - are equal, or sum to exactly r (the sum must come out 0, not r), or to r -+ 1."""
    n = 1 << k
    d = (n >> (t + 1)) if dif else (1 << t)
    x = np.array(unpack(random_residues(seed, n // 2)), dtype=object).reshape(n // (2 * d), d)
    x = np.where((x < 2) | (x > R - 2), 5, x)      # (so that r - x -+ 1 stays inside [0, r))
    want = {"equal": x, "sum=r": R - x, "sum=r-1": R - x - 1, "sum=r+1": R - x + 1}[kind]
    if not dif:
        tw_inv = twiddles(k, not inverse)[np.arange(d) << (k - 1 - t)]     # y = want / w^e
        want = want * tw_inv % R
    a = np.empty((n // (2 * d), 2, d), dtype=object)
    a[:, 0, :] = x
    a[:, 1, :] = want
    return [int(v) for v in a.reshape(n)]


@functools.lru_cache(maxsize=None)
def pass_case(k, dif, inverse, t0, g, kind, prev=None):
    """(input residues, expected residues) of one pass over the stages t0 .. t0 + g - 1.  `prev` = the (t0, g) of the passes
    before it, for the kind "random": its input is what those passes make of the first one's, so the last pass's expectation is
    the whole chain's."""
    n = 1 << k
    seed = (k * 64 + t0) * 16 + KINDS.index(kind) + (4096 if inverse else 0) + (8192 if dif else 0)
    if kind == "random":
        if prev:
            v = pass_case(k, dif, inverse, prev[-1][0], prev[-1][1], "random", prev[:-1])[1]
        else:
            v = unpack(random_residues(1000 + k, n))
    elif kind == "random2":
        v = unpack(random_residues(seed, n))
    elif kind == "zero":
        v = [0] * n
    elif kind == "r-1":
        v = [R - 1] * n
    elif kind.startswith("one@"):
        v = [0] * n
        v[{"0": 0, "1": 1 % n, "n/2": n // 2, "n-1": n - 1}[kind[4:]]] = 1
    else:
        v = _partner_inputs(kind, k, dif, inverse, t0, seed)
    assert all(0 <= x < R for x in v)
    return v, stages(v, k, dif, inverse, t0, g)


def _gapped(polys, n, stride):
    """the polynomials laid out `stride` apart, every word of the gaps the sentinel"""
    data = np.full((len(polys) * stride, 8), SENTINEL, dtype=np.uint32)
    for p, v in enumerate(polys):
        data[p * stride:p * stride + n] = _words(v)
    return data


def _assert_polys(data, want, n, stride, what):
    for p, w in enumerate(want):
        got = data[p * stride:p * stride + n]
        if not np.array_equal(got, _words(w)):
            bad = [i for i, (a, b) in enumerate(zip(unpack(got), unpack(_words(w)))) if a != b]
            raise AssertionError("%s: polynomial %d differs at %d indices, first %s" % (what, p, len(bad), bad[:8]))
        assert (data[p * stride + n:(p + 1) * stride] == SENTINEL).all(), (what, "gap written", p)


def check_passes(lib, form, k, dif, inverse):
    """every pass of the chain alone, on every kind of input, one polynomial per launch (stride n) and three different ones
    (stride n + 5, the gaps untouched); then the whole chain.  Returns the number of launches compared."""
    n = 1 << k
    chosen, ps = plan(lib, k, 1, dif, form)
    assert chosen == form
    runs = 0
    prev = ()
    for i, (t0, g, *_rest) in enumerate(ps):
        cases = [pass_case(k, dif, inverse, t0, g, kind, prev if kind == "random" else None) for kind in KINDS]
        for j, (v, want) in enumerate(cases):
            data = _gapped([v], n, n)
            assert chain(lib, k, form, dif, inverse, data, n, first=i, count=1) == 0
            _assert_polys(data, [want], n, n, (FORM_NAMES[form], k, dif, inverse, "pass", i, KINDS[j]))
            runs += 1
        for j in range(0, len(cases), 3):
            three = cases[j:j + 3]
            data = _gapped([c[0] for c in three], n, n + GAP)
            assert chain(lib, k, form, dif, inverse, data, n + GAP, first=i, count=1) == 0
            _assert_polys(data, [c[1] for c in three], n, n + GAP, (FORM_NAMES[form], k, dif, inverse, "pass", i, KINDS[j:j + 3]))
            runs += 1
        prev = prev + ((t0, g),)
    # the whole chain: the first pass's random input, the last pass's expectation - and, with three, two more kinds whose
    # expectation is all the stages
    v0 = pass_case(k, dif, inverse, ps[0][0], ps[0][1], "random", ())[0]
    last = pass_case(k, dif, inverse, ps[-1][0], ps[-1][1], "random", prev[:-1])[1]
    data = _gapped([v0], n, n)
    assert chain(lib, k, form, dif, inverse, data, n) == 0
    _assert_polys(data, [last], n, n, (FORM_NAMES[form], k, dif, inverse, "chain"))
    others = [pass_case(k, dif, inverse, 0, ps[0][1], kind)[0] for kind in ("sum=r", "one@n-1")]
    data = _gapped([v0] + others, n, n + GAP)
    assert chain(lib, k, form, dif, inverse, data, n + GAP) == 0
    _assert_polys(data, [last] + [stages(v, k, dif, inverse, 0, k) for v in others], n, n + GAP, (FORM_NAMES[form], k, dif, inverse, "chain of 3"))
    # an empty range launches nothing
    data = _gapped([v0], n, n)
    assert chain(lib, k, form, dif, inverse, data, n, first=len(ps), count=1) == 0
    _assert_polys(data, [v0], n, n, "empty range")
    return runs + 2


# ------------------------------------------------------------------------------------------------ c. chain options
def _mulm(a, b):
    """what the kernel's mul makes of two residues: a b / 2^256"""
    return [x * y * MONT_INV % R for x, y in zip(a, b)]


def _words(vals_or_words):
    return vals_or_words if isinstance(vals_or_words, np.ndarray) else pack(vals_or_words)


def transform_words(words, k, dif, inverse):
    return pack(stages(unpack(words), k, dif, inverse, 0, k)) if k < 14 else c_fft(words, k, dif, inverse)


def check_options(lib, form, k, dif):
    """pre, post, minus and src of a chain of three polynomials `n + 5` apart (DIF with the forward twiddles, DIT with the
    inverse ones)"""
    n = 1 << k
    batch, stride = 3, n + GAP
    inverse = 1 - dif
    over = pack([R, R + 1, (1 << 256) - 1])       # values >= r
    what = (FORM_NAMES[form], k, dif)
    T = lambda w: transform_words(w, k, dif, inverse)
    mulm = lambda w, tab: pack(_mulm(unpack(w), tab))
    subm = lambda w, m: pack([(a - b) % R for a, b in zip(unpack(w), unpack(m))])
    polys = [random_residues(50 + 3 * k + p, n) for p in range(batch)]
    pre = unpack(random_residues(60 + k, n))
    post = unpack(random_residues(61 + k, n))
    plain = [T(v) for v in polys]
    # pre: at the load of the first pass, by global position; post: at the store of the last
    with_pre = [T(mulm(v, pre)) for v in polys]
    data = _gapped(polys, n, stride)
    assert chain(lib, k, form, dif, inverse, data, stride, pre=pack(pre)) == 0
    _assert_polys(data, with_pre, n, stride, what + ("pre",))
    data = _gapped(polys, n, stride)
    assert chain(lib, k, form, dif, inverse, data, stride, post=pack(post)) == 0
    _assert_polys(data, [mulm(v, post) for v in plain], n, stride, what + ("post",))
    # minus, its own stride: subtracted after post, in the order of the store
    ms = n + 3
    minus = [random_residues(70 + 3 * k + p, n) for p in range(batch)]
    mbuf = _gapped(minus, n, ms)
    data = _gapped(polys, n, stride)
    assert chain(lib, k, form, dif, inverse, data, stride, pre=pack(pre), post=pack(post), minus=mbuf, minus_stride=ms) == 0
    _assert_polys(data, [subm(mulm(v, post), m) for v, m in zip(with_pre, minus)], n, stride, what + ("pre post minus",))
    data = _gapped(polys, n, stride)
    assert chain(lib, k, form, dif, inverse, data, stride, minus=mbuf, minus_stride=ms) == 0
    _assert_polys(data, [subm(v, m) for v, m in zip(plain, minus)], n, stride, what + ("minus",))
    # src: the first `valid` elements of a row of `valid + 7`, zero beyond; the 7 are >= r: neither read nor flagged
    for valid in (1, n // 2 - 3, n - 1, n):
        ss = valid + 7
        src = np.empty((batch * ss, 8), dtype=np.uint32)
        want = []
        for p in range(batch):
            v = random_residues(80 + p, valid)
            src[p * ss:p * ss + valid] = v
            src[p * ss + valid:(p + 1) * ss] = over[np.arange(7) % 3]
            want.append(T(np.concatenate([v, np.zeros((n - valid, 8), dtype=np.uint32)])))
        data = np.full((batch * stride, 8), SENTINEL, dtype=np.uint32)     # (what `data` held is not read at all)
        assert chain(lib, k, form, dif, inverse, data, stride, src=src, src_stride=ss, src_valid=valid) == 0, what + ("src", valid)
        _assert_polys(data, want, n, stride, what + ("src", valid))
        # a value >= r at the first and at the last valid index, of the first and of the last polynomial: the flag
        for o, (p, idx) in enumerate(((0, 0), (batch - 1, valid - 1), (1, valid - 1))):
            s2 = src.copy()
            s2[p * ss + idx] = over[o]
            data = np.full((batch * stride, 8), SENTINEL, dtype=np.uint32)
            assert chain(lib, k, form, dif, inverse, data, stride, src=s2, src_stride=ss, src_valid=valid) == ZK_BAD_SCALAR, \
                what + ("flag", valid, p, idx)
            for q in range(batch):
                assert (data[q * stride + n:(q + 1) * stride] == SENTINEL).all()
        # r - 1 at those places is a scalar like any other
        s2 = src.copy()
        s2[0] = s2[(batch - 1) * ss + valid - 1] = pack([R - 1])[0]
        data = np.full((batch * stride, 8), SENTINEL, dtype=np.uint32)
        assert chain(lib, k, form, dif, inverse, data, stride, src=s2, src_stride=ss, src_valid=valid) == 0


def check_size_one_chain(lib):
    """k = 0 has no pass to carry a table or a source: refused; without them it is the identity"""
    one = pack([5])
    tab = pack([7])
    for form in (LATENCY, SMALL, BIG):
        d = one.copy()
        assert chain(lib, 0, form, 1, 0, d, 1) == 0 and np.array_equal(d, one)
        for kw in ({"pre": tab}, {"post": tab}, {"src": tab, "src_stride": 1, "src_valid": 1}):
            d = one.copy()
            assert chain(lib, 0, form, 1, 0, d, 1, status=True, **kw) == ZK_ERR_INVALID_ARGUMENT
            assert np.array_equal(d, one)
    d = one.copy()
    assert chain(lib, 0, MID, 1, 0, d, 1, status=True) == ZK_ERR_INVALID_ARGUMENT      # (no mid form below 2^11)
    d = pack(range(1024))
    assert chain(lib, 10, MID, 1, 0, d, 1024, status=True) == ZK_ERR_INVALID_ARGUMENT
    assert np.array_equal(d, pack(range(1024)))


# ------------------------------------------------------------------------------------------------ d. tile forms from 2^14
LARGE = [(LATENCY, 14, 1), (LATENCY, 15, 1), (LATENCY, 16, 1), (LATENCY, 16, 2)] + \
        [(SMALL, k, 1) for k in (14, 16, 17, 20)] + [(MID, k, 1) for k in (17, 20, 21)] + [(BIG, k, 1) for k in (17, 20, 21)]


def check_large(lib, form, k, batch, dif, inverse=0):
    n = 1 << k
    if form == MID:
        # Any cut of the k stages into passes gives these bytes: what the order of mid's passes decides is which pass has the
        # contiguous tile (s = 0, log_cw = 0: 64 KiB in one piece) - the one of 11 stages, last in a DIF chain, first in a DIT chain.
        ps = plan(lib, k, batch, dif, form)[1]
        s_of = lambda t0, g: k - t0 - g if dif else t0
        assert [(g, lcw) for (t0, g, lcw, *_r) in ps if s_of(t0, g) == 0] == [(11, 0)], ps
    x = random_residues(900 + k + 7 * batch, batch * n)
    data = x.copy()
    assert chain(lib, k, form, dif, inverse, data, n) == 0
    for p in range(batch):
        want = c_fft(x[p * n:(p + 1) * n], k, dif, inverse)
        got = data[p * n:(p + 1) * n]
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).any(axis=1))[0]
            raise AssertionError("%s 2^%d dif=%d inverse=%d polynomial %d: %d elements differ, first %s" % (FORM_NAMES[form], k, dif, inverse, p, bad.size, bad[:8]))


# ------------------------------------------------------------------------------------------------ e. zk_ntt_run_dev
INV, COSET, IN_BR, OUT_BR = 1, 2, 4, 8


def refused(flags):
    """forward coset from bit-reversed input, inverse coset into bit-reversed output (csrc/zkamd.cpp ntt_run_dev)"""
    return (flags & (INV | COSET | IN_BR)) == (COSET | IN_BR) or (flags & (INV | COSET | OUT_BR)) == (INV | COSET | OUT_BR)


def check_run_dev(lib, k, alloc, batch=3):
    """all sixteen combinations of the four flags on `batch` polynomials: the oracle's four bellman operations on the same bytes
    (linear, with tables in Montgomery form: residues in, residues out) between the two bit reversals - IN_BITREV: element i
    sits at position bitrev(i); OUT_BITREV: the same on the way out."""
    n = 1 << k
    br = bitrev_perm(k)
    x = random_residues(300 + k, batch * n)
    x[0] = 0
    x[-1] = pack([R - 1])[0]
    nbytes = x.size * 4
    dptr, upload, download, free = alloc(nbytes)
    t = C.c_void_p()
    lib.check(lib.zk_ntt_create(k, 0, C.byref(t)))
    accepted = 0
    try:
        for flags in range(16):
            upload(dptr, x.view(np.uint8).reshape(-1))
            st = lib.zk_ntt_run_dev(t, dptr, batch, flags)
            lib.check(lib.zk_synchronize())
            got = np.frombuffer(download(dptr, nbytes), dtype=np.uint32).reshape(batch * n, 8)
            if k and refused(flags):
                assert st == ZK_ERR_INVALID_ARGUMENT, (k, flags)
                assert np.array_equal(got, x), (k, flags, "a refused call wrote")
                continue
            assert st == 0, (k, flags)
            if k == 0:
                assert np.array_equal(got, x), (flags, "a transform of one point is the identity")
            accepted += 1
            for p in range(batch):
                v = x[p * n:(p + 1) * n]
                if flags & IN_BR:
                    v = v[br]
                w = np.frombuffer(cport.fft(np.ascontiguousarray(v).tobytes(), k, bool(flags & INV), bool(flags & COSET), 2),
                                  dtype=np.uint32).reshape(n, 8)
                if flags & OUT_BR:
                    w = w[br]
                assert np.array_equal(got[p * n:(p + 1) * n], w), (k, flags, p)
        # no polynomial: nothing runs, whatever the flags
        upload(dptr, x.view(np.uint8).reshape(-1))
        for flags in (0, INV | COSET, COSET | IN_BR):
            assert lib.zk_ntt_run_dev(t, dptr, 0, flags) == 0
        lib.check(lib.zk_synchronize())
        assert download(dptr, nbytes) == x.tobytes()
    finally:
        lib.zk_ntt_free(t)
        free(dptr)
    return accepted


# ------------------------------------------------------------------------------------------------ f. the tables
def check_tables(lib, k):
    n = 1 << k
    w, winv = omega(k), pow(omega(k), -1, R)
    ginv, ninv = pow(GEN, -1, R), pow(n, -1, R)
    zinv = pow(pow(GEN, n, R) - 1, -1, R)
    assert pow(w, n, R) == 1 and (k == 0 or pow(w, n // 2, R) == R - 1)
    m = lambda v: v * MONT % R                                   # the Montgomery form
    br = [bitrev(i, k) for i in range(n)]
    want = {
        "tw_fwd": [m(pow(w, e, R)) for e in range(n // 2)],
        "tw_inv": [m(pow(winv, e, R)) for e in range(n // 2)],
        # g^bitrev(pos) / n; s1_plain carries one more factor 2^256 (it lifts a plain input), s2 one fewer (it leaves plain values)
        "s1_plain": [m(m(pow(GEN, br[p], R) * ninv)) for p in range(n)],
        "s1_mont": [m(pow(GEN, br[p], R) * ninv) for p in range(n)],
        "s2": [pow(ginv, br[p], R) * ninv % R for p in range(n)],
        "dt": [m(br[p] * ninv) for p in range(n)],
        "sc_plain": [m(ninv * zinv)] * n,
        "sc_mont": [ninv * zinv % R] * n,
        "coset_fwd": [m(pow(GEN, i, R)) for i in range(n)],
        "coset_inv": [m(pow(ginv, i, R) * ninv) for i in range(n)],
        "consts": [m(ninv), m(zinv)],
    }
    assert set(want) == set(TABLES)
    for name in TABLES:
        got = table(lib, k, name)
        assert len(got) == len(want[name]), (k, name, len(got))
        assert got == want[name], (k, name, [i for i, (a, b) in enumerate(zip(got, want[name])) if a != b][:8])
    fn = lib.dll.zk_hook_ntt_table
    nb = C.c_size_t(0)
    assert fn(k, len(TABLES), None, 0, C.byref(nb)) == ZK_ERR_INVALID_ARGUMENT
