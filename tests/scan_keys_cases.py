"""Builders and expectations for tests/test_scan_keys.py (zk_scan_keys_*, zk_confidential_scan_keys, zk_anonymous_scan_keys).

The extrinsics come from the builders of tests/scan_cases.py, and so do the expectations: for every pair (extrinsic i, key k) the 16
bytes scan_cases.expected_confidential / expected_anonymous computes with oracle/jubjub.py for dec_key k.  The hits a call must return
are exactly the pairs whose expectation is not 16 zero bytes, in (xt, key) order, with those bytes."""
import struct

import scan_cases as sc
from oracle import jubjub as jj

STRANGERS = sc.fs(103, 3)          # three keys no case pays or is paid by
EDGE = [1, 2, jj.FS_MOD - 1, 1 << 251, int("7" * 63, 16)]
# FS_MOD has 252 bits, so FS_MOD - 1 and 2^251 set bit 251 - the window at 252 holds it alone - and 0x0777..7 is below FS_MOD;
# its bits 0111 0111 .. put a carry into every Booth window
assert jj.FS_MOD.bit_length() == 252 and all(0 < k < jj.FS_MOD for k in EDGE) and EDGE[2] >> 251 == EDGE[3] >> 251 == 1
CYCLE = sc.fs(104, 5)              # the five keys of the lane-layout block


def expected_hits(kind, xts, dks, logs):
    """[(xt, key, 16 bytes)] for the keys `dks`, by the oracle alone.  A pair whose extrinsic does not carry dk G - the first thing
    expected_* looks at, and what it answers 16 zero bytes to - is decided here with one dk G per key instead of one per pair."""
    expected = sc.expected_confidential if kind == "confidential" else sc.expected_anonymous
    carried = (lambda x: (x["enc_key_sender"], x["enc_key_recipient"])) if kind == "confidential" else (lambda x: x["enc_keys"])
    enc = [jj.write_point(jj.mul(sc.G, dk)) for dk in dks]
    out = []
    for i, x in enumerate(xts):
        for k, dk in enumerate(dks):
            if enc[k] not in carried(x):
                continue
            # (computed once for an extrinsic that several blocks hold: the lane-layout cases repeat theirs)
            memo = (kind, id(x), dk, logs.limit, len(logs.tab))
            if memo not in _expected:
                _expected[memo] = (x, expected(x, dk, logs))
            e = _expected[memo][1]
            if e != bytes(16):
                out.append((i, k, e))
    return out


_expected = {}   # (kind, id of the xt dict, dk, limit, table size) -> (the dict, kept alive so that its id stays its own; 16 bytes)


def edge_cases(lib, amounts):
    """every key of EDGE as the sender of one transfer and the recipient of another: key j pays key j + 1"""
    specs = [(EDGE[j], EDGE[(j + 1) % 5], amounts[j], j) for j in range(5)]
    return sc.confidential_xts(lib, specs, seed=31), list(amounts) + list(range(5))


def lane_layout_cases(lib):
    """70 transfers k_j -> k_(j+1) over the five keys of CYCLE: 140 hits - the multiplication lanes fill two waves and twelve lanes
    of a third - and 350 points, so the decode lanes end inside their sixth wave; the same block with a stranger's transfer between
    every two; a block whose only hit is its last extrinsic.  Returns (cycle, mixed, last, candidates)."""
    cycle = sc.confidential_xts(lib, [(CYCLE[j % 5], CYCLE[(j + 1) % 5], 100 + 7 * j, j % 9) for j in range(70)], seed=32)
    strangers = sc.confidential_xts(lib, [(sc.ALICE, sc.BOB, 1, 1)] * 69, seed=33)
    mixed = [x for pair in zip(cycle, strangers + [None]) for x in pair][:-1]   # the same 70, a stranger's between every two
    last = [(sc.ALICE, sc.BOB, 2, 1)] * 5 + [(sc.BOB, CYCLE[3], 77, 1)]
    cand = [100 + 7 * j for j in range(70)] + list(range(9)) + [77]
    return cycle, mixed, sc.confidential_xts(lib, last, seed=34), cand


def ring_of(lib, placed):
    """twelve keys and values: `placed` maps a position to (decryption key, value); strangers with 0 elsewhere"""
    import zero_chain_amd as zk
    others = sc.other_keys(lib, 12)
    mine = dict(zip(placed, zk.jubjub_base_mul([dk for dk, _ in placed.values()], lib=lib))) if placed else {}
    return ([mine.get(k, others[k]) for k in range(12)], [placed[k][1] if k in placed else 0 for k in range(12)])


def ring_cases(lib, amounts):
    """for every amount a: three keys of the set at positions 0, 5 and 11 as sender (-a), recipient (+a) and decoy (0), and a ring
    in which one key appears twice (+a and a decoy's 0) and another once (-a); then a ring without any key of the set.  The key set is
    [WALLET, ALICE, BOB].  Returns (xts, candidates)."""
    w, a_, b = sc.WALLET, sc.ALICE, sc.BOB
    specs = []
    for a in amounts:
        specs += [ring_of(lib, {0: (w, -a), 5: (a_, a), 11: (b, 0)}), ring_of(lib, {2: (b, a), 7: (w, -a), 9: (b, 0)})]
    specs.append(ring_of(lib, {}))
    return sc.anonymous_xts(lib, specs, seed=35), list(amounts) + [0]


def random_block(lib, rng, n_keys, n_strangers, n, amount):
    """n confidential and n anonymous extrinsics among n_keys keys of a set and n_strangers others.  Returns (dks of the set, cx, ax,
    hits_c, hits_a) where hits_* list (xt, key, role or members, values) from the plaintexts the block was built from:
    confidential values = (amount, fee), anonymous values = {position: signed value}."""
    dks = sc.fs(105, n_keys + n_strangers)
    number = {dk: k for k, dk in enumerate(dks[:n_keys])}
    cspecs, hits_c = [], []
    for i in range(n):
        s, r = rng.choice(dks), rng.choice(dks)
        a, f = amount(), rng.randrange(1000)
        cspecs.append((s, r, a, f))
        roles = {}
        if s in number:
            roles[number[s]] = sc.SENDER
        if r in number:
            roles[number[r]] = roles.get(number[r], 0) | sc.RECIPIENT
        hits_c += [(i, k, roles[k], (a, f)) for k in sorted(roles)]
    import zero_chain_amd as zk
    enc = dict(zip(dks, zk.jubjub_base_mul(dks, lib=lib)))
    aspecs, hits_a = [], []
    for i in range(n):
        ring = rng.sample(dks, 12)
        a = amount()
        s, t = rng.sample(range(12), 2)
        vals = [0] * 12
        vals[s], vals[t] = -a, a
        aspecs.append(([enc[dk] for dk in ring], vals))
        hits_a += sorted((i, number[dk], 1 << p, vals[p]) for p, dk in enumerate(ring) if dk in number)
    return dks[:n_keys], sc.confidential_xts(lib, cspecs, seed=36), sc.anonymous_xts(lib, aspecs, seed=37), hits_c, hits_a


def confidential_bytes(role, values, limit):
    a, f = values
    val = lambda v: (1, v) if v < limit else (0, 0)
    s, fee, rec = (val(a) if role & 1 else (0, 0)), (val(f) if role & 1 else (0, 0)), (val(a) if role & 2 else (0, 0))
    return struct.pack("<BBBBIII", role, s[0] | fee[0] << 1 | rec[0] << 2, 0, 0, s[1], fee[1], rec[1])


def anonymous_bytes(members, v, limit):
    ok = abs(v) < limit
    return struct.pack("<HBBIq", members, ok, 0, 0, v if ok else 0)
